"""Every seed kernel on the dense, adjacent and clustered lists of tests/seed_cases.py, and the minima kernels on the images whose
maxima are the case, -m gpu.  Bit for bit against the CPU oracle (ol.segment_arrival, ol.merge_arrival, ol.find_local_minima),
tests/merge_tree_ref.py and tests/lake_stats_ref.py, and against the closed forms where there is one (every pixel a seed: pixel
p carries p + 1; followed by its reverse: 2 H W - p).  tests/test_seed_cases_cpu.py proves that the inputs reach the regimes.

Which form a transform takes (csrc/ws_segment.hip, run_fused): a context starts out expecting a strictly increasing list, so on a
FRESH context such a list at W % 4 == 0 takes the seed tables (k_seed_tables, the resolve's TABLES branch); any other width paints
(k_paint_sorted).  A list that is not strictly increasing is refused by the tables, painted, and flips the context's expectation:
the sorted list that follows is painted too (k_paint_sorted on a dense sorted list at W % 4 == 0), which flips it back, and the one
after that takes the tables again.  `_four_forms` walks through exactly that.
"""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import lake_stats_ref as ls
import merge_tree_ref as mt
import oracle_lib as ol
import seed_cases as sc
import strided

pytestmark = pytest.mark.gpu

S = sc.segment_cases()
M = sc.minima_cases()


def _ids(cs):
    return [c[0] for c in cs]


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def dev(pkg):
    return importlib.import_module("rustronomy_watershed_amd.device")


def _u64(seeds):
    return np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1, 2))


def _to_dev(eng, img, seeds):
    import torch
    t_img = torch.from_numpy(np.ascontiguousarray(img)).to(eng.device)
    t_seeds = torch.from_numpy(np.asarray(seeds, dtype=np.int64).reshape(-1, 2).astype(np.int32)).to(eng.device).contiguous()
    return t_img, t_seeds


def _np32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- the oracle, once per (case, question) ------------------------------------------------------------------------------------------

_WANT = {}


def _cached(key, make):
    if key not in _WANT:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _WANT[key] = v
    return _WANT[key]


def want_segment(name, img, seeds, edge=False, shift=False):
    s = np.asarray(seeds, dtype=np.int64).reshape(-1, 2) + (1 if edge and shift else 0)
    return _cached((name, "seg", edge, shift), lambda: ol.segment_arrival(img, s, edge=edge))


def closed_form(name, img, seeds):
    """The labels where they are known without any flood, else None."""
    h, w = img.shape
    if name.startswith("S1/"):
        return (np.arange(h * w, dtype=np.uint64) + 1).reshape(h, w)
    if "/all_then_reversed/" in name:
        return (2 * h * w - np.arange(h * w, dtype=np.uint64)).reshape(h, w)
    return None


def _check_segment(got, case, tag):
    name, img, seeds, _ = case
    want = want_segment(name, img, seeds)
    assert got.shape == want.shape and (got == want).all(), (name, tag, int((got != want).sum()))
    cf = closed_form(name, img, seeds)
    if cf is not None:
        assert (got == cf).all(), (name, tag, "closed form")


def _twin(case):
    """The same seeds in another order, and the oracle's labels for it (another colouring: the colours are list positions)."""
    name, img, seeds, _ = case
    tw = sc.shuffled(seeds, 7)
    return tw, _cached((name, "twin"), lambda: ol.segment_arrival(img, tw))


def _four_forms(case, run):
    """run(seeds) -> labels, on ONE fresh context: the list; its shuffled twin; the list again, twice (module docstring)."""
    name, img, seeds, facts = case
    _check_segment(run(seeds), case, "fresh context")
    if len(seeds) < 2:
        return
    tw, want_tw = _twin(case)
    got = run(tw)
    assert (got == want_tw).all(), (name, "shuffled twin", int((got != want_tw).sum()))
    _check_segment(run(seeds), case, "after the twin")
    _check_segment(run(seeds), case, "prediction flipped back")


# ---- ws_segment (host, u64 seeds) and ws_segment_device, every S case -----------------------------------------------------------------

@pytest.mark.parametrize("case", S, ids=_ids(S))
def test_host_segment_on_dense_seed_lists(pkg, case):
    name, img, seeds, _ = case
    ctx = pkg.api.Context(0)
    try:
        ws = pkg.TransformBuilder.new().set_context(ctx).build_segmenting()
        _four_forms(case, lambda s: ws.transform(img, _u64(s)))
    finally:
        ctx.close()


@pytest.mark.parametrize("case", S, ids=_ids(S))
def test_device_segment_on_dense_seed_lists(pkg, dev, case):
    name, img, seeds, _ = case
    eng = dev.DeviceEngine(0)

    def run(s):
        t_img, t_seeds = _to_dev(eng, img, s)
        return _np32(eng.segment(t_img, t_seeds))

    _four_forms(case, run)


AT_A = sc.by_family("S1", "S2", "S3", "S4", "S5", "S6", "S7", shape="A")


@pytest.mark.parametrize("case", AT_A, ids=_ids(AT_A))
def test_sweep_engine_segment_on_dense_seed_lists(pkg, case):
    name, img, seeds, _ = case
    ctx = pkg.api.Context(0)
    try:
        for engine in (pkg.ENGINE_SWEEP, pkg.ENGINE_FUSED):
            ws = pkg.TransformBuilder.new().set_context(ctx).set_engine(engine).build_segmenting()
            _check_segment(ws.transform(img, _u64(seeds)), case, engine)
    finally:
        ctx.close()


EDGE = sc.by_family("S1", "S2", shape="ABC")


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("case", EDGE, ids=_ids(EDGE))
def test_segment_with_edge_correction_on_dense_seed_lists(pkg, dev, case, shift):
    name, img, seeds, _ = case
    want = want_segment(name, img, seeds, edge=True, shift=shift)
    ctx = pkg.api.Context(0)
    try:
        b = pkg.TransformBuilder.new().set_context(ctx).enable_edge_correction().shift_seeds_into_padded_plane(shift)
        got = b.build_segmenting().transform(img, _u64(seeds))
        assert got.shape == want.shape and (got == want).all(), (name, shift, "host")
    finally:
        ctx.close()
    eng = dev.DeviceEngine(0)
    t_img, t_seeds = _to_dev(eng, img, seeds)
    got = _np32(eng.segment(t_img, t_seeds, edge=True, seed_shift=shift))
    assert (got == want).all(), (name, shift, "device")
    if shift and name.startswith("S1/"):      # every image pixel a seed, on its own pixel: the ring stays empty
        h, w = img.shape
        cf = np.zeros((h + 2, w + 2), dtype=np.uint64)
        cf[1:-1, 1:-1] = (np.arange(h * w, dtype=np.uint64) + 1).reshape(h, w)
        assert (got == cf).all(), name


# ---- ws_segment_batch_device, stacked ------------------------------------------------------------------------------------------------

def test_segment_batch_stack_of_a_full_an_empty_and_a_half_full_slice(pkg, dev):
    import torch
    eng = dev.DeviceEngine(0)
    full, half = sc.case_named("S1/B/"), sc.case_named("S2/B/half/")
    h, w = sc.SHAPES["B"]
    imgs = [full[1], sc.image("plateau", h, w, 77), half[1]]
    lists = [full[2], np.zeros((0, 2), dtype=np.int64), half[2]]
    assert (h * w) % 128 == 0 and w % 4 == 0 and len(lists[0]) == h * w > sc.TAB_CHUNK      # slice_first subtracts 10240 seeds
    offs = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    cube = torch.from_numpy(np.stack(imgs)).to(eng.device)
    allseeds = torch.from_numpy(np.concatenate(lists).astype(np.int32)).to(eng.device).contiguous()
    got = _np32(eng.segment_batch(cube, allseeds, offs))
    batch_relax = eng.stats()["launches_relax"]
    loop_relax = 0
    for k in range(3):
        t_img, t_seeds = _to_dev(eng, imgs[k], lists[k])
        one = _np32(eng.segment(t_img, t_seeds))
        loop_relax += eng.stats()["launches_relax"]
        assert (got[k] == one).all(), k
        assert (got[k] == ol.segment_arrival(imgs[k], lists[k])).all(), k
    assert (got[0] == closed_form(full[0], full[1], full[2])).all() and not got[1].any()
    assert 0 < batch_relax < loop_relax, (batch_relax, loop_relax)      # one transform for the stack, not three


# ---- the seam-repair flow: the tall pass-0 kernel's seed bits ---------------------------------------------------------------------------

SEAM = sc.by_family("S2", "S3", shape="G")


@pytest.mark.parametrize("case", SEAM, ids=_ids(SEAM))
def test_segment_seam_repair_flow_on_dense_seed_lists(pkg, dev, case):
    name, img, seeds, facts = case
    assert facts["form"] == "tables"
    eng = dev.DeviceEngine(0)
    eng.ctx.set_seam_repair_min_pixels(1)
    try:
        t_img, t_seeds = _to_dev(eng, img, seeds)
        for rep in range(2):
            _check_segment(_np32(eng.segment(t_img, t_seeds)), case, ("seam", rep))
            st = eng.stats()
            assert st["launches_relax"] == st["relax_passes"] + 1, st      # pass 1 was two launches (bands, strips): the seam flow ran
        tw, want_tw = _twin(case)
        t_img, t_tw = _to_dev(eng, img, tw)
        assert (_np32(eng.segment(t_img, t_tw)) == want_tw).all(), (name, "painted seeds through the seam flow")
    finally:
        eng.ctx.set_seam_repair_min_pixels(0)


# ---- merging: unions, per-level lists, history, the tree and its statistics with n_colours up to H * W --------------------------------

MERGING = [sc.case_named("S1/A/"), sc.case_named("S2/A/half/"), sc.case_named("S3/D/chunk1/"), sc.case_named("S6/A/rows_then_reversed/"),
           # colour 2 (overwritten by the reversed copy) in a one-lake tile, below a lake id in the thousands (test_final_merge_cases_cpu.py)
           sc.case_named("S6/A/all_then_reversed/"), sc.case_named("S6/A/half_then_reversed/"),
           sc.case_named("S6/C/all_then_reversed/"), sc.case_named("S6/C/half_then_reversed/")]


def want_planes(case):
    name, img, seeds, _ = case
    return _cached((name, "planes"), lambda: mt.oracle_planes(img, seeds))


def want_lists(case, merging):
    name, img, seeds, _ = case

    def make():
        per_level = {}
        (ol.merge_arrival if merging else ol.segment)(img, seeds, hook=lambda l, m, i, c: per_level.__setitem__(l, ol.find_lake_sizes(c)))
        return per_level
    return _cached((name, "lists", merging), make)


def _lists_device(pkg, eng, t_img, t_seeds, merging, cap):
    import torch
    h, w = t_img.shape
    lakes = torch.full((max(cap, 1) + 2, 2), -7, dtype=torch.int64, device=eng.device)      # two guard records behind cap
    n = ctypes.c_size_t(0)
    offsets, uncol = np.zeros(256, dtype=np.uint64), np.zeros(255, dtype=np.uint64)
    opt = eng.options(254, False)
    rc = pkg._ffi.lib().ws_transform_to_list_device(eng.ctx.handle, int(merging), t_img.data_ptr(), h, w, w, t_seeds.data_ptr(), t_seeds.shape[0],
                                                    ctypes.byref(opt), lakes.data_ptr(), cap, ctypes.byref(n), offsets.ctypes.data, uncol.ctypes.data)
    torch.cuda.synchronize()
    rec = lakes.cpu().numpy()
    assert (rec[max(cap, 1):] == -7).all(), "records written behind the capacity"
    return rc, n.value, rec[:cap].view(np.uint64), offsets, uncol


def _check_lists(rec, n_lakes, offsets, uncol, want, n_pixels, tag):
    """Every level's records scattered into the dense vector of lib.rs:628-635 (index 0: the uncoloured pixels) against the oracle's
    find_lake_sizes; a colour appears once in a level."""
    assert n_lakes == offsets[255] and sorted(want) == list(range(255)), tag
    for lvl in range(255):
        part = rec[int(offsets[lvl]):int(offsets[lvl + 1])]
        colours = part[:, 0].astype(np.int64)
        assert (colours > 0).all() and len(np.unique(colours)) == len(colours), (tag, lvl)
        assert (colours <= n_pixels).all(), (tag, lvl)
        dense = np.zeros(n_pixels + 1, dtype=np.uint64)
        dense[colours] = part[:, 1]
        dense[0] = uncol[lvl]
        assert (dense == want[lvl]).all(), (tag, lvl)


@pytest.mark.parametrize("case", MERGING, ids=_ids(MERGING))
def test_merge_device_final_labels_on_dense_seed_lists(pkg, dev, case):
    name, img, seeds, _ = case
    eng = dev.DeviceEngine(0)
    t_img, t_seeds = _to_dev(eng, img, seeds)
    want = _cached((name, "merge"), lambda: ol.merge_arrival(img, seeds))
    for rep in range(2):
        got = _np32(eng.merge(t_img, t_seeds))
        assert (got == want).all(), (name, rep, int((got != want).sum()))
    assert (want == want_planes(case)[0][-1]).all()      # (the two oracles agree on the last plane)


# (a list longer than the plane has colours above H * W: the per-level vector of find_lake_sizes has H * W + 1 entries, the
# reference panics on such a colour, lib.rs:628-635, and the oracle's copy of it must not be handed one)
AT_A_MERGING = [c for c in MERGING if c[3]["shape"] == "A" and len(c[2]) <= c[1].size]


@pytest.mark.parametrize("merging", [1, 0])
@pytest.mark.parametrize("case", AT_A_MERGING, ids=_ids(AT_A_MERGING))
def test_transform_to_list_device_on_dense_seed_lists(pkg, dev, case, merging):
    name, img, seeds, _ = case
    eng = dev.DeviceEngine(0)
    t_img, t_seeds = _to_dev(eng, img, seeds)
    want = want_lists(case, merging)
    count = sum(int(np.count_nonzero(v[1:])) for v in want.values())      # the capacity comes from the oracle
    rc, n, rec, offsets, uncol = _lists_device(pkg, eng, t_img, t_seeds, merging, count)
    assert rc == 0 and n == count, (name, merging, rc, n, count)
    _check_lists(rec, n, offsets, uncol, want, img.size, (name, merging))
    rc, n, _, _, _ = _lists_device(pkg, eng, t_img, t_seeds, merging, count - 1)      # one short
    assert rc == pkg._ffi.WS_ERR_CAPACITY and n == count, (name, merging, rc, n)
    rc, n, rec, offsets, uncol = _lists_device(pkg, eng, t_img, t_seeds, merging, count)      # ... and the context works on
    assert rc == 0 and n == count
    _check_lists(rec, n, offsets, uncol, want, img.size, (name, merging, "again"))


def test_transform_to_list_device_from_the_live_list_with_every_pixel_a_colour(pkg, dev):
    case = sc.case_named("S1/A/")
    name, img, seeds, _ = case
    eng = dev.DeviceEngine(0)
    L = pkg._ffi.lib()
    assert L.ws_ctx_set_live_list_min_colours(eng.ctx.handle, 1) == 0
    try:
        t_img, t_seeds = _to_dev(eng, img, seeds)
        want = want_lists(case, 1)
        count = sum(int(np.count_nonzero(v[1:])) for v in want.values())
        rc, n, rec, offsets, uncol = _lists_device(pkg, eng, t_img, t_seeds, 1, count)
        assert rc == 0 and n == count, (rc, n, count)
        _check_lists(rec, n, offsets, uncol, want, img.size, name)
    finally:
        assert L.ws_ctx_set_live_list_min_colours(eng.ctx.handle, 0) == 0


HISTORY_LEVELS = [0, 1, 127, 254]


@pytest.mark.parametrize("case", MERGING, ids=_ids(MERGING))
def test_transform_history_device_on_dense_seed_lists(pkg, dev, case):
    name, img, seeds, _ = case
    eng = dev.DeviceEngine(0)
    t_img, t_seeds = _to_dev(eng, img, seeds)
    planes, _ = want_planes(case)
    got = _np32(eng.transform_history(t_img, t_seeds, levels=HISTORY_LEVELS, merging=True))
    for k, lvl in enumerate(HISTORY_LEVELS):
        assert (got[k] == planes[lvl]).all(), (name, "merging", lvl, int((got[k] != planes[lvl]).sum()))
    seg = {}
    ol.segment(img, seeds, hook=lambda l, m, i, c: seg.__setitem__(l, c.copy()) if l in HISTORY_LEVELS else None)
    got = _np32(eng.transform_history(t_img, t_seeds, levels=HISTORY_LEVELS, merging=False))
    for k, lvl in enumerate(HISTORY_LEVELS):
        assert (got[k] == seg[lvl]).all(), (name, "segmenting", lvl)
    assert (seg[254] == want_segment(name, img, seeds)).all()


@pytest.mark.parametrize("case", MERGING, ids=_ids(MERGING))
def test_merge_tree_and_stats_device_on_dense_seed_lists(pkg, dev, case):
    import torch
    name, img, seeds, _ = case
    eng = dev.DeviceEngine(0)
    t_img, t_seeds = _to_dev(eng, img, seeds)
    planes, ps = want_planes(case)
    parent, death, area, leaves, vals, ex = mt.tree_from_planes(planes, ps)
    want_tree = np.stack([parent, death, area, leaves], axis=1)
    if name.startswith("S1/"):
        assert ex[1:].all() and len(seeds) == img.size      # n_colours == H * W, every one of them a lake of its own at first
    tree, labels = eng.merge_tree(t_img, t_seeds, want_labels=True)
    torch.cuda.synchronize()
    tree = _np32(tree)
    bad = np.flatnonzero((tree != want_tree).any(axis=1))
    assert bad.size == 0, (name, bad[:5], tree[bad[:5]], want_tree[bad[:5]])
    assert (_np32(labels) == want_segment(name, img, seeds)).all()
    mt.check_invariants(tree[:, 0], tree[:, 1], tree[:, 2], tree[:, 3], vals, ex)
    u16 = np.random.default_rng(5).integers(0, 65536, img.shape, dtype=np.uint16)
    u16.reshape(-1)[::97] = 65535
    u16.reshape(-1)[5::89] = 0
    want = ls.stats_from_planes(planes, ps, ls.plane_weights(img, u16, False), death, ex)
    tree2, raw = eng.merge_tree_stats(t_img, t_seeds, weights=torch.from_numpy(u16.view(np.int16)).to(eng.device))
    torch.cuda.synchronize()
    assert (_np32(tree2) == want_tree).all(), name
    rec = ls.from_raw(raw.cpu().numpy())
    assert ls.mismatch(rec, want) is None, (name, ls.mismatch(rec, want))


# ---- one local group of three ranks: colour_bias and ws_block_begin with dense seeds -----------------------------------------------------

TILED = [sc.case_named("S1/A/"), sc.case_named("S2/A/half/"), sc.case_named("S2/A/seven_eighths/")]


@pytest.fixture(scope="module")
def group3(pkg):
    g = importlib.import_module("rustronomy_watershed_amd.group").Group.local(3)
    yield g
    g.close()


@pytest.mark.parametrize("case", TILED, ids=_ids(TILED))
def test_segment_tiled_over_three_ranks_on_dense_seed_lists(pkg, group3, case):
    name, img, seeds, facts = case
    assert facts["form"] == "tables"      # the fast form of the row blocks: every rank builds its tables from its part of the list
    ffi = pkg._ffi
    h, w = img.shape
    img = np.ascontiguousarray(img)

    def run(s, merging):
        s = _u64(s)
        out = np.full((h, w), 7, dtype=np.uint64)
        opt = ffi.Options(254)
        rounds = ctypes.c_uint32(0)
        rc = ffi.lib().ws_segment_tiled(group3._h, img.ctypes.data, h, w, w, s.ctypes.data, len(s), ctypes.byref(opt), int(merging), out.ctypes.data,
                                        ctypes.byref(rounds))
        assert rc == 0, (name, rc, ffi.lib().ws_group_last_error(group3._h))
        return out

    _check_segment(run(seeds, False), case, "tiled")
    tw, want_tw = _twin(case)
    assert (run(tw, False) == want_tw).all(), (name, "general form")
    want = _cached((name, "merge"), lambda: ol.merge_arrival(img, seeds))
    got = run(seeds, True)
    assert (got == want).all(), (name, "tiled merging", int((got != want).sum()))


# ---- ws_find_local_minima and ws_find_local_minima_device, every M case -----------------------------------------------------------------

GUARD = 0xA5A5A5A5


def _want_minima(case):
    name, img, facts = case
    return _cached((name, "minima"), lambda: ol.find_local_minima(img).astype(np.int64).reshape(-1, 2))


def _layout(case):
    """(backing bytes, offset of pixel (0, 0), row stride)."""
    name, img, facts = case
    h, w = img.shape
    if "offset" in facts:
        backing, off, _ = strided.embed(img, facts["offset"], facts["row_stride"], ("random", 3))
        return backing, off, facts["row_stride"]
    return np.ascontiguousarray(img).reshape(-1), 0, w


@pytest.mark.parametrize("case", M, ids=_ids(M))
def test_find_local_minima_host_on_constructed_maxima(pkg, case):
    name, img, facts = case
    h, w = img.shape
    want = _want_minima(case)
    if facts["want"] is not None:
        assert want.shape == facts["want"].shape and (want == facts["want"]).all()
    backing, off, rs = _layout(case)
    ctx = pkg.api.Context(0)
    L = pkg._ffi.lib()
    try:
        found = len(want)
        for cap in sorted({found + 3, found, max(found - 1, 0), 0}, reverse=True):
            out = np.full((cap + 2, 2), GUARD, dtype=np.uint64)
            n = ctypes.c_size_t(12345)
            rc = L.ws_find_local_minima(ctx.handle, backing.ctypes.data + off, h, w, rs, out.ctypes.data, cap, ctypes.byref(n))
            assert n.value == found, (name, cap, n.value, found)
            assert rc == (0 if cap >= found else pkg._ffi.WS_ERR_CAPACITY), (name, cap, rc)
            k = min(cap, found)
            assert (out[:k] == want[:k].astype(np.uint64)).all(), (name, cap)      # content and order
            assert (out[k:] == GUARD).all(), (name, cap, "words behind the list were written")
    finally:
        ctx.close()


@pytest.mark.parametrize("case", M, ids=_ids(M))
def test_find_local_minima_device_on_constructed_maxima(pkg, dev, case):
    import torch
    name, img, facts = case
    h, w = img.shape
    want = _want_minima(case)
    backing, off, rs = _layout(case)
    eng = dev.DeviceEngine(0)
    L = pkg._ffi.lib()
    d_img = torch.from_numpy(backing).to(eng.device)
    found = len(want)
    for cap in sorted({found + 3, found, max(found - 1, 0), 0}, reverse=True):
        out = torch.full((cap + 2, 2), -23, dtype=torch.int32, device=eng.device)
        n = ctypes.c_size_t(12345)
        rc = L.ws_find_local_minima_device(eng.ctx.handle, d_img.data_ptr() + off, h, w, rs, out.data_ptr(), cap, ctypes.byref(n))
        torch.cuda.synchronize()
        assert n.value == found, (name, cap, n.value, found)
        assert rc == (0 if cap >= found else pkg._ffi.WS_ERR_CAPACITY), (name, cap, rc)
        got = out.cpu().numpy()
        k = min(cap, found)
        assert (got[:k] == want[:k]).all(), (name, cap)
        assert (got[k:] == -23).all(), (name, cap, "words behind the list were written")


# ---- ws_segment_minima, _u32 and _device on M1, M2 and M5 -----------------------------------------------------------------------------

FROM_MINIMA = [c for c in M if c[2]["family"] in ("M1", "M2", "M5") and c[1].shape in ((9, 2080), (9, 2084), (40, 2049), (66, 130), (5, 8))
               and "offset" not in c[2]]


@pytest.mark.parametrize("case", FROM_MINIMA, ids=_ids(FROM_MINIMA))
def test_segment_minima_on_constructed_maxima(pkg, dev, case):
    import torch
    name, img, facts = case
    h, w = img.shape
    seeds = _want_minima(case)
    want = _cached((name, "seg"), lambda: ol.segment_arrival(img, seeds))
    ctx = pkg.api.Context(0)
    try:
        ws = pkg.TransformBuilder.new().set_context(ctx).build_segmenting()
        for rep in range(2):      # the second run knows the dense count of the first (minima_found_before)
            got, got_seeds = ws.transform_from_minima(img, want_seeds=True)
            assert got_seeds.shape == seeds.shape and (got_seeds == seeds.astype(np.uint64)).all(), (name, rep)
            assert (got == want).all(), (name, rep, int((got != want).sum()))
            got32 = ws.transform_from_minima(img, labels_u32=True)      # (no list asked for)
            assert got32.dtype == np.uint32 and (got32 == want).all(), (name, rep)
        pair = ws.transform(img, ws.find_local_minima(img))      # the call pair
        assert (pair == want).all(), name
    finally:
        ctx.close()
    eng = dev.DeviceEngine(0)
    t_img = torch.from_numpy(np.ascontiguousarray(img)).to(eng.device)
    for rep in range(2):
        labels, n, t_seeds = eng.segment_minima(t_img, want_seeds=True)
        assert n == len(seeds) and (t_seeds.cpu().numpy() == seeds).all(), (name, rep)
        assert (_np32(labels) == want).all(), (name, rep)
        labels, n = eng.segment_minima(t_img)
        assert n == len(seeds) and (_np32(labels) == want).all(), (name, rep)
