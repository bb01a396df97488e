"""The tiled transforms (csrc/ws_tiled.hip over the block steps of csrc/ws_block_api.hip) on the inputs of tests/tiled_cases.py:
blocks of one or two owned rows, seeds on seam and halo rows, ranks without seeds, a corridor that crosses every seam 45 times, a
plateau, lakes linked across blocks, edge correction down to a rank that owns only the virtual ring row -- every case in the fast
form and in the general one, bit for bit against the CPU oracle; no tolerance anywhere.  tests/test_tiled_cases_cpu.py proves on
the oracle that the inputs reach these regimes and runs the same protocol on the numpy stand-in.

Local groups on device 0, ONE per world (2, 3, 4, 8) for the whole module.

Which form a call took.  tiled_rank counts the collective steps every rank takes part in (*exchange_rounds):

  fast     1 (the vote) + S (halo swaps: until no rank receives a row that differs from the one it holds, S >= 1) + 1 (the table)
  general  1 (the vote) + R0 (stamp rounds: until no rank's relaxation changed anything) + R1 (label rounds, the same rule)

and + 1 with merging (the pair table) in both.  So both forms take 3 (+ 1) rounds at least, and a bound on the count of ONE call
cannot tell them apart.  What the code implies: the general form's loops end with a round in which nothing changed, so a case in
which any pixel beyond the seeds is coloured has R0 >= 2 and R1 >= 2 (a first round that changes nothing would leave the painted
seeds as the result): 5 (+ 1) rounds at least.  And for a field and the SAME seeds in another order (the /shuffled twins) both
forms walk through the same stamp planes -- local convergence, swap, again; stamps do not depend on colours -- so "no received
row differs" after relaxation t implies "relaxation t + 1 changes nothing", and "relaxation t changed nothing" implies "no
received row differs" after it: S <= R0 <= S + 1, hence

  rounds(general twin) - rounds(fast) = (R0 - S) + (R1 - 1) >= R1 - 1 >= 1   whenever a pixel beyond the seeds is coloured.

A "fast" case that quietly took the general form would show the twin's count exactly.  Where nothing floods (a field of two
rows has no interior) both forms take 3 rounds and the count cannot separate them: those cases take the fast form because every
condition of tiled_rank holds by construction -- no explicit colours (the host call found the rows sorted), w % 4 == 0, two
local rows or more on every rank (one owned row and a halo row at least), a strictly increasing list (ws_block_begin's check)
-- which tests/test_tiled_cases_cpu.py asserts of every /fast case.  The /wide twins are another field (the old last column
becomes interior), so no relation between their count and the fast case's is asserted: they take the general form because
w % 4 != 0 fails the first test of tiled_rank on every rank.
"""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import oracle_lib as ol
import tiled_cases as tc

pytestmark = pytest.mark.gpu

WORLDS = (2, 3, 4, 8)
U64_MAX = (1 << 64) - 1


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def groups(pkg):
    grp_mod = importlib.import_module("rustronomy_watershed_amd.group")
    gs = {world: grp_mod.Group.local(world) for world in WORLDS}
    yield gs
    for g in gs.values():
        g.close()


def _ids(cs):
    return [c[0] for c in cs]


def _u64(seeds):
    return np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1, 2))


# ---- the oracle, once per case ----------------------------------------------------------------------------------------------------

_WANT = {}


def _plain(case):
    """(image, seeds) of the call without edge correction that the case equals, and the oracle call's own arguments."""
    name, img, seeds, _ = case
    edge, shift = tc.edge_options(name)
    if edge and shift:
        pad, moved = tc.padded_equivalent(img, seeds, True)
        return pad, moved, False
    return img, np.asarray(seeds, dtype=np.int64).reshape(-1, 2), edge


def want_segment(case):
    key = (case[0], "seg")
    if key not in _WANT:
        img, seeds, edge = _plain(case)
        # (ol.segment and ol.segment_arrival are the same labels: tests/test_oracle_golden.py; the first takes edge correction)
        _WANT[key] = ol.segment(img, seeds, edge=True) if edge else ol.segment_arrival(img, seeds)
    return _WANT[key]


def want_merge(case, level):
    key = (case[0], "merge", level)
    if key not in _WANT:
        img, seeds, edge = _plain(case)
        _WANT[key] = ol.merge_arrival(img, seeds, max_level=level, edge=edge)
    return _WANT[key]


def want_lists(case, merging, level=254):
    key = (case[0], "lists", merging, level)
    if key not in _WANT:
        img, seeds, edge = _plain(case)
        per_level = {}
        (ol.merge_arrival if merging else ol.segment)(img, seeds, max_level=level, edge=edge,
                                                      hook=lambda l, m, i, c: per_level.__setitem__(l, ol.find_lake_sizes(c)))
        _WANT[key] = per_level
    return _WANT[key]


def floods(case):
    """A pixel beyond the seeds is coloured."""
    img, seeds, _ = _plain(case)
    return int(np.count_nonzero(want_segment(case))) > len(np.unique(seeds, axis=0))


def merge_levels(name):
    return tc.LINKED_LEVELS if name.startswith("f/") or name.startswith("g/f/") else (254, 120, 60)


# ---- the calls ----------------------------------------------------------------------------------------------------------------------

def segment_tiled(pkg, g, case, merging=False, max_level=254, seeds=None, edge=None, shift=None, expect=0):
    name, img, case_seeds, _ = case
    ffi = pkg._ffi
    e_, s_ = tc.edge_options(name)
    edge, shift = (e_ if edge is None else edge), (s_ if shift is None else shift)
    s = _u64(case_seeds if seeds is None else seeds)
    img = np.ascontiguousarray(img)
    h, w = img.shape
    e = 2 if edge else 0
    out = np.full((h + e, w + e), 7, dtype=np.uint64)
    opt = ffi.Options(max_level, int(edge), 0, 0, int(shift))
    rounds = ctypes.c_uint32(0)
    rc = ffi.lib().ws_segment_tiled(g._h, img.ctypes.data, h, w, w, s.ctypes.data, len(s), ctypes.byref(opt), int(merging), out.ctypes.data,
                                    ctypes.byref(rounds))
    assert rc == expect, (name, rc, ffi.lib().ws_group_last_error(g._h))
    return out, rounds.value


def lists_tiled(pkg, g, case, merging, max_level=254, seeds=None, edge=None, shift=None, expect=0):
    name, img, case_seeds, _ = case
    ffi = pkg._ffi
    e_, s_ = tc.edge_options(name)
    edge, shift = (e_ if edge is None else edge), (s_ if shift is None else shift)
    s = _u64(case_seeds if seeds is None else seeds)
    img = np.ascontiguousarray(img)
    h, w = img.shape
    cap = (max_level + 1) * (len(s) + 1)      # every colour alive at every level: the most there can be
    rec = np.zeros((cap, 2), dtype=np.uint64)
    n_lakes = ctypes.c_size_t(0)
    offsets, uncol = np.zeros(max_level + 2, dtype=np.uint64), np.zeros(max_level + 1, dtype=np.uint64)
    opt = ffi.Options(max_level, int(edge), 0, 0, int(shift))
    rc = ffi.lib().ws_transform_to_list_tiled(g._h, int(merging), img.ctypes.data, h, w, w, s.ctypes.data, len(s), ctypes.byref(opt), rec.ctypes.data, cap,
                                              ctypes.byref(n_lakes), offsets.ctypes.data, uncol.ctypes.data, None)
    assert rc == expect, (name, rc, ffi.lib().ws_group_last_error(g._h))
    return rec, n_lakes.value, offsets, uncol


def segment_tiled2d(pkg, g, case, py, px, merging=False, max_level=254, seeds=None, edge=False, shift=False, expect=0):
    name, img, case_seeds, _ = case
    ffi = pkg._ffi
    s = _u64(case_seeds if seeds is None else seeds)
    img = np.ascontiguousarray(img)
    h, w = img.shape
    e = 2 if edge else 0
    out = np.full((h + e, w + e), 7, dtype=np.uint64)
    opt = ffi.Options(max_level, int(edge), 0, 0, int(shift))
    rounds = ctypes.c_uint32(0)
    rc = ffi.lib().ws_segment_tiled2d(g._h, img.ctypes.data, h, w, w, s.ctypes.data, len(s), ctypes.byref(opt), py, px, int(merging), out.ctypes.data,
                                      ctypes.byref(rounds))
    assert rc == expect, (name, rc, ffi.lib().ws_group_last_error(g._h))
    return out, rounds.value


def check_lists(rec, n_lakes, offsets, uncol, want, n_pixels, tag):
    """Every level's records scattered into the dense vector of lib.rs:628-635 (index 0: the uncoloured pixels) against the oracle's
    find_lake_sizes; a colour appears once in a level."""
    levels = len(uncol)
    assert n_lakes == offsets[levels] and sorted(want) == list(range(levels)), tag
    for lvl in range(levels):
        part = rec[int(offsets[lvl]):int(offsets[lvl + 1])]
        colours = part[:, 0].astype(np.int64)
        assert (colours > 0).all() and len(np.unique(colours)) == len(colours), (tag, lvl)
        dense = np.zeros(n_pixels + 1, dtype=np.uint64)
        dense[colours] = part[:, 1].astype(np.uint64)
        dense[0] = uncol[lvl]
        assert (dense == want[lvl]).all(), (tag, lvl)


# ---- host forms: ws_segment_tiled -----------------------------------------------------------------------------------------------

ALL = tc.all_cases()
BY_NAME = {c[0]: c for c in ALL}


@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_segmenting_in_row_blocks_equals_the_oracle(pkg, groups, case):
    name, _, _, world = case
    got, rounds = segment_tiled(pkg, groups[world], case)
    want = want_segment(case)
    assert got.shape == want.shape and (got == want).all(), (name, int((got != want).sum()))
    # (module docstring) the vote, one swap or one stamp round, the table or one label round; the general form's loops end with an
    # idle round each, so where anything floods they take two rounds at least
    assert rounds >= (5 if tc.form_of(name) != "fast" and floods(case) else 3), (name, rounds)


@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_merging_in_row_blocks_equals_the_oracle(pkg, groups, case):
    name, _, _, world = case
    _, seg_rounds = segment_tiled(pkg, groups[world], case)
    for level in merge_levels(name):
        got, rounds = segment_tiled(pkg, groups[world], case, merging=True, max_level=level)
        want = want_merge(case, level)
        assert (got == want).all(), (name, level, int((got != want).sum()))
        if level == 254:
            assert rounds == seg_rounds + 1, (name, rounds, seg_rounds)      # ONE exchange joins the lakes, whatever their shape


SHUFFLED_PAIRS = [(c, BY_NAME[c[0][: -len("fast")] + "shuffled"]) for c in ALL if tc.form_of(c[0]) == "fast" and c[0][: -len("fast")] + "shuffled" in BY_NAME]


@pytest.mark.parametrize("fast,twin", SHUFFLED_PAIRS, ids=[c[0][: -len("/fast")] for c, _ in SHUFFLED_PAIRS])
def test_the_sorted_list_takes_the_fast_form_and_its_shuffled_twin_the_general_one(pkg, groups, fast, twin):
    # (module docstring) the same stamps in both forms: S <= R0 <= S + 1, and the general form's label rounds R1 >= 2 where anything
    # floods, against the fast form's one table exchange
    g = groups[fast[3]]
    _, r_fast = segment_tiled(pkg, g, fast)
    _, r_general = segment_tiled(pkg, g, twin)
    assert r_fast >= 3 and r_general >= 3
    if floods(fast):
        assert r_general >= r_fast + 1, (fast[0], r_fast, r_general)
        _, m_fast = segment_tiled(pkg, g, fast, merging=True)
        _, m_general = segment_tiled(pkg, g, twin, merging=True)
        assert (m_fast, m_general) == (r_fast + 1, r_general + 1)
    else:
        assert tc.is_strictly_increasing(fast[2], fast[1].shape[1] + (2 if tc.edge_options(fast[0])[0] else 0))


# ---- host forms: ws_transform_to_list_tiled ---------------------------------------------------------------------------------------

LIST_CASES = tc.all_cases("aef")


@pytest.mark.parametrize("merging", [1, 0])
@pytest.mark.parametrize("case", LIST_CASES, ids=_ids(LIST_CASES))
def test_lists_of_a_field_in_row_blocks_equal_the_oracle(pkg, groups, case, merging):
    name, img, seeds, world = case
    for level in ((254, 60) if name.startswith("f/") else (254,)):
        rec, n_lakes, offsets, uncol = lists_tiled(pkg, groups[world], case, merging, max_level=level)
        check_lists(rec, n_lakes, offsets, uncol, want_lists(case, merging, level), img.size, (name, merging, level))


# ---- 2-D forms ----------------------------------------------------------------------------------------------------------------------

TILE_CASES = tc.all_cases("cf")


def _grids(world):
    return ((world, 1), (2, 2))


@pytest.mark.parametrize("case", TILE_CASES, ids=_ids(TILE_CASES))
def test_2d_tiles_of_a_host_field_equal_the_oracle(pkg, groups, case):
    name, _, _, world = case
    for py, px in _grids(world):
        g = groups[py * px]
        got, rounds = segment_tiled2d(pkg, g, case, py, px)
        assert (got == want_segment(case)).all(), (name, py, px)
        assert rounds >= 2
        for level in merge_levels(name):
            got, _ = segment_tiled2d(pkg, g, case, py, px, merging=True, max_level=level)
            assert (got == want_merge(case, level)).all(), (name, py, px, level)


@pytest.mark.parametrize("merging", [1, 0])
@pytest.mark.parametrize("case", TILE_CASES, ids=_ids(TILE_CASES))
def test_lists_of_a_field_in_2d_tiles_equal_the_oracle_and_the_halo_ring_holds_the_owners_labels(pkg, groups, case, merging):
    import torch
    name, img, seeds, world = case
    ffi = pkg._ffi
    dev = torch.device("cuda", 0)
    H, W = img.shape
    want = want_segment(case)
    for py, px in _grids(world):
        g = groups[py * px]
        field = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
        s = torch.from_numpy(np.asarray(seeds, dtype=np.int64).reshape(-1, 2).astype(np.int32)).to(dev)
        blocks, spans, keep = g.make_blocks2d(field, s, py, px)
        cap = 255 * (len(seeds) + 1)
        lakes = torch.zeros((cap, 2), dtype=torch.int64, device=dev)
        n_lakes = ctypes.c_size_t(0)
        offsets, uncol = np.zeros(256, dtype=np.uint64), np.zeros(255, dtype=np.uint64)
        opt = ffi.Options(254)
        rc = ffi.lib().ws_transform_to_list_tiled2d_device(g._h, H, W, py, px, len(seeds), blocks, ctypes.byref(opt), int(merging), lakes.data_ptr(), cap,
                                                           ctypes.byref(n_lakes), offsets.ctypes.data, uncol.ctypes.data, None)
        assert rc == 0, (name, rc, ffi.lib().ws_group_last_error(g._h))
        check_lists(lakes.cpu().numpy().view(np.uint64), n_lakes.value, offsets, uncol, want_lists(case, merging), H * W, (name, py, px, merging))
        # the tiles hold the segmenting labels; every tile's halo ring holds the owner's (the ring's four corners are nobody's stencil)
        for (r0, r1, lo, hi), (c0, c1, clo, chi), lab in spans:
            L = lab.cpu().numpy().view(np.uint32)
            assert (L[r0 - lo:r1 - lo, c0 - clo:c1 - clo] == want[r0:r1, c0:c1]).all(), (name, py, px)
            if lo < r0:
                assert (L[0, c0 - clo:c1 - clo] == want[lo, c0:c1]).all()
            if hi > r1:
                assert (L[-1, c0 - clo:c1 - clo] == want[hi - 1, c0:c1]).all()
            if clo < c0:
                assert (L[r0 - lo:r1 - lo, 0] == want[r0:r1, clo]).all()
            if chi > c1:
                assert (L[r0 - lo:r1 - lo, -1] == want[r0:r1, chi - 1]).all()


# ---- device form: ws_segment_tiled_device on the blocks of Group.make_blocks ----------------------------------------------------

DEVICE_CASES = [c for c in tc.all_cases("af") if tc.form_of(c[0]) in ("fast", "wide")]      # (make_blocks takes a strictly increasing list)


@pytest.mark.parametrize("case", DEVICE_CASES, ids=_ids(DEVICE_CASES))
def test_device_row_blocks_equal_the_oracle_and_the_halo_rows_hold_the_owners_labels(pkg, groups, case):
    import torch
    name, img, seeds, world = case
    g = groups[world]
    dev = torch.device("cuda", 0)
    H, W = img.shape
    field = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
    s = torch.from_numpy(np.asarray(seeds, dtype=np.int64).reshape(-1, 2).astype(np.int32)).to(dev)
    blocks, spans, keep = g.make_blocks(H, lambda lo, hi, rank: field[lo:hi].contiguous(), s)

    def check(want, tag):
        for r0, r1, lo, lab in spans:
            L = lab.cpu().numpy().view(np.uint32)
            hi = lo + L.shape[0]
            assert (L[r0 - lo:r1 - lo] == want[r0:r1]).all(), (name, tag, r0)
            if lo < r0:
                assert (L[0] == want[lo]).all(), (name, tag, "top halo", r0)
            if hi > r1:
                assert (L[-1] == want[hi - 1]).all(), (name, tag, "bottom halo", r0)

    rounds = g.segment_tiled_device(H, W, len(seeds), blocks)
    check(want_segment(case), "segmenting")
    assert rounds >= (5 if tc.form_of(name) != "fast" and floods(case) else 3)
    for level in merge_levels(name):
        g.segment_tiled_device(H, W, len(seeds), blocks, max_level=level, merging=True)
        check(want_merge(case, level), level)


# ---- seeds outside the plane: WS_ERR_SEED_OOB, and the group works on -------------------------------------------------------------

def _oob_lists(rng, good, h, w):
    """(tag, list, edge_correction, seed_shift).  With both options set the engine adds 1 to every coordinate: 2^64 - 1 wraps to 0,
    which is inside every plane; 2^32 + 2 is inside only after truncation to 32 bits."""
    good = _u64(good)
    mid = len(good) // 2
    shuffled = good[rng.permutation(len(good))]
    out = []
    for tag, bad in (("row", (U64_MAX, 3)), ("col", (3, U64_MAX))):
        b = np.array([bad], dtype=np.uint64)
        out.append((f"{tag} 2^64-1 last", np.concatenate([good, b]), 1, 1))       # "row": rows still sorted, the binary-search branch
        out.append((f"{tag} 2^64-1 amid a shuffled list", np.concatenate([shuffled[:mid], b, shuffled[mid:]]), 1, 1))
    for tag, bad in (("row", ((1 << 32) + 2, 1)), ("col", (1, (1 << 32) + 2))):
        b = np.array([bad], dtype=np.uint64)
        for edge, shift in ((1, 1), (1, 0), (0, 0)):
            out.append((f"{tag} 2^32+2 last edge={edge} shift={shift}", np.concatenate([good, b]), edge, shift))
            out.append((f"{tag} 2^32+2 amid edge={edge} shift={shift}", np.concatenate([good[:mid], b, good[mid:]]), edge, shift))
    return [(t, np.ascontiguousarray(l), e, s) for t, l, e, s in out]


@pytest.mark.parametrize("entry", ["ws_segment_tiled", "ws_segment_tiled2d", "ws_transform_to_list_tiled"])
def test_a_seed_outside_the_plane_is_refused_before_any_addition_can_wrap(pkg, groups, entry):
    # The host forms used to test coordinate + shift against the plane: with both options set every 2^64 - 1 list below came back
    # WS_OK from all three entry points, the seed painted at row or column 0 -- but for the row-sorted list that ends in
    # (2^64 - 1, 3), which the row-block forms refused by accident (the binary search handed the wrapped seed to the last rank,
    # whose block steps found its local row out of range) and ws_segment_tiled2d accepted.  The 2^32 + 2 lists were always refused.
    ffi = pkg._ffi
    g = groups[4]
    h, w = 24, 32
    img = cases.field(h, w, 6)
    good = _u64(ol.find_local_minima(img))
    case = ("oob/fast", img, good, 4)
    want = ol.segment_arrival(img, good)
    for tag, lst, edge, shift in _oob_lists(np.random.default_rng(5), good, h, w):
        if entry == "ws_segment_tiled":
            segment_tiled(pkg, g, case, seeds=lst, edge=edge, shift=shift, expect=ffi.WS_ERR_SEED_OOB)
        elif entry == "ws_segment_tiled2d":
            segment_tiled2d(pkg, g, case, 2, 2, seeds=lst, edge=edge, shift=shift, expect=ffi.WS_ERR_SEED_OOB)
        else:
            lists_tiled(pkg, g, case, 1, seeds=lst, edge=edge, shift=shift, expect=ffi.WS_ERR_SEED_OOB)
        # the group is usable after the error: one good transform through the same entry point
        if entry == "ws_segment_tiled":
            got, _ = segment_tiled(pkg, g, case)
            assert (got == want).all(), tag
        elif entry == "ws_segment_tiled2d":
            got, _ = segment_tiled2d(pkg, g, case, 2, 2)
            assert (got == want).all(), tag
        else:
            rec, n_lakes, offsets, uncol = lists_tiled(pkg, g, case, 1)
            check_lists(rec, n_lakes, offsets, uncol, want_lists(case, 1), h * w, tag)


def test_other_errors_leave_the_groups_usable(pkg, groups):
    ffi = pkg._ffi
    for world in WORLDS:
        g = groups[world]
        case = next(c for c in ALL if c[0].startswith("b/") and c[3] == world and tc.form_of(c[0]) == "fast")
        name, img, seeds, _ = case
        few = np.ascontiguousarray(img[: world - 1])          # fewer rows than ranks
        segment_tiled(pkg, g, ("few/fast", few, seeds[:1] * 0, world), expect=ffi.WS_ERR_BAD_ARG)
        bad = np.concatenate([_u64(seeds), np.array([[img.shape[0], 0]], dtype=np.uint64)])      # one row below the plane
        segment_tiled(pkg, g, case, seeds=bad, expect=ffi.WS_ERR_SEED_OOB)
        lists_tiled(pkg, g, case, 1, seeds=bad, expect=ffi.WS_ERR_SEED_OOB)
        rec, n_lakes, offsets, uncol = lists_tiled(pkg, g, case, 1)
        assert n_lakes > 7
        opt = ffi.Options(254)
        im = np.ascontiguousarray(img)
        s = _u64(seeds)
        n2 = ctypes.c_size_t(0)
        rc = ffi.lib().ws_transform_to_list_tiled(g._h, 1, im.ctypes.data, im.shape[0], im.shape[1], im.shape[1], s.ctypes.data, len(s), ctypes.byref(opt),
                                                  rec.ctypes.data, 7, ctypes.byref(n2), offsets.ctypes.data, uncol.ctypes.data, None)
        assert rc == ffi.WS_ERR_CAPACITY and n2.value == n_lakes      # a record buffer that is too small: the count is still reported
        got, _ = segment_tiled(pkg, g, case)
        assert (got == want_segment(case)).all(), name
        got, _ = segment_tiled(pkg, g, case, merging=True, max_level=120)
        assert (got == want_merge(case, 120)).all(), name


def test_the_single_context_entry_points_refuse_the_same_lists(pkg):
    # ws_segment and ws_transform_to_list compare the raw coordinate with ph - shift before they add the shift (k_narrow_seeds)
    ffi = pkg._ffi
    L = ffi.lib()
    h, w = 24, 32
    img = cases.field(h, w, 6)
    good = _u64(ol.find_local_minima(img))
    ws = pkg.api.TransformBuilder().build_segmenting()
    ctx = ws._ctx().handle
    want = ol.segment_arrival(img, good)
    want_l = {}
    ol.merge_arrival(img, good, hook=lambda l, m, i, c: want_l.__setitem__(l, ol.find_lake_sizes(c)))
    cap = 255 * (len(good) + 2)
    rec = np.zeros((cap, 2), dtype=np.uint64)
    offsets, uncol = np.zeros(256, dtype=np.uint64), np.zeros(255, dtype=np.uint64)
    for tag, lst, edge, shift in _oob_lists(np.random.default_rng(5), good, h, w):
        e = 2 if edge else 0
        out = np.zeros((h + e, w + e), dtype=np.uint64)
        opt = ffi.Options(254, edge, 0, 0, shift)
        assert L.ws_segment(ctx, img.ctypes.data, h, w, w, lst.ctypes.data, len(lst), ctypes.byref(opt), out.ctypes.data) == ffi.WS_ERR_SEED_OOB, tag
        n_lakes = ctypes.c_size_t(0)
        assert L.ws_transform_to_list(ctx, 1, img.ctypes.data, h, w, w, lst.ctypes.data, len(lst), ctypes.byref(opt), rec.ctypes.data, cap, ctypes.byref(n_lakes),
                                      offsets.ctypes.data, uncol.ctypes.data) == ffi.WS_ERR_SEED_OOB, tag
        opt = ffi.Options(254)
        out = np.zeros((h, w), dtype=np.uint64)
        assert L.ws_segment(ctx, img.ctypes.data, h, w, w, good.ctypes.data, len(good), ctypes.byref(opt), out.ctypes.data) == 0
        assert (out == want).all(), tag
    n_lakes = ctypes.c_size_t(0)
    assert L.ws_transform_to_list(ctx, 1, img.ctypes.data, h, w, w, good.ctypes.data, len(good), ctypes.byref(opt), rec.ctypes.data, cap, ctypes.byref(n_lakes),
                                  offsets.ctypes.data, uncol.ctypes.data) == 0
    check_lists(rec, n_lakes.value, offsets, uncol, want_l, h * w, "after the errors")
