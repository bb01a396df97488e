"""The 2-D tiled transforms (tiled2d_rank in csrc/ws_tiled.hip over the block steps of csrc/ws_block_api.hip) on the inputs of
tests/tiled2d_cases.py: the row families transposed, tiles of one or two columns, seeds on the pixels where a row seam meets a
column seam, corridors that cross every column seam 40 times and wind round the crossing point, plateaus with ties on seams, lakes
linked through other tiles, edge correction down to a tile that owns only the virtual ring column -- every case on every grid it
lists, through the host call, the device call (owned rectangles AND halo rings), the lists and the tree with its catalogue, bit for
bit against the CPU oracle; no tolerance anywhere.  tests/test_tiled2d_cases_cpu.py proves on the oracle that the inputs reach
these regimes and runs the same protocol on the numpy stand-in.

Local groups on device 0, ONE per world (2, 3, 4, 6, 8) for the whole module.  Family t is run whole (no case is thinned out).

Rounds (family w).  tiled2d_rank counts the collective steps every rank takes part in (*exchange_rounds): the rounds of the stamp
loop (relax to local convergence, swap the ring, "did any rank change anything"), the rounds of the label loop, and one more with
merging (the pair table).  A stamp reaches another tile only through a swap, a swap carries it across ONE seam, and the corridor's
path is unique: the K crossings from the seed to the far end take K swaps, in K rounds that each changed something, and the loop
ends only with a round in which nothing changed -- K + 1 rounds at least.  The label loop takes one round at least.  Hence

  exchange_rounds >= K + 2,   K + 3 with merging

-- a lower bound from the code, not a measurement.  (The round after the K-th swap still floods the last stretch of the corridor,
so the stamp loop in fact takes K + 2; the bound asserted is the weaker one that does not lean on where the corridor ends.)
"""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import lake_stats_ref as ls
import oracle_lib as ol
import tiled_cases as tc
import tiled2d_cases as t2
from test_gpu_tiled_edges import check_lists, segment_tiled2d

pytestmark = pytest.mark.gpu

WORLDS = (2, 3, 4, 6, 8)


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


@pytest.fixture(scope="module")
def eng(pkg):
    import torch
    with torch.cuda.stream(torch.cuda.Stream(0)):
        yield importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


def _params(letters):
    ps = t2.pairs(letters)
    return pytest.mark.parametrize("case,grid", ps, ids=[t2.pair_id(c, g) for c, g in ps])


# ---- the oracle, once per case ------------------------------------------------------------------------------------------------------

_WANT = {}


def _plain(case):
    """(image, seeds) of the call without edge correction that the case equals: family z through tiled_cases.padded_equivalent."""
    name, img, seeds, _ = case
    edge, shift = tc.edge_options(name)
    if edge:
        return tc.padded_equivalent(img, seeds, shift)
    return img, np.asarray(seeds, dtype=np.int64).reshape(-1, 2)


def want_segment(case):
    key = (case[0], "seg")
    if key not in _WANT:
        _WANT[key] = ol.segment_arrival(*_plain(case))
    return _WANT[key]


def want_merge(case, level):
    key = (case[0], "merge", level)
    if key not in _WANT:
        _WANT[key] = ol.merge_arrival(*_plain(case), max_level=level)
    return _WANT[key]


def want_lists(case, merging):
    key = (case[0], "lists", merging)
    if key not in _WANT:
        per_level = {}
        (ol.merge_arrival if merging else ol.segment)(*_plain(case), hook=lambda l, m, i, c: per_level.__setitem__(l, ol.find_lake_sizes(c)))
        _WANT[key] = per_level
    return _WANT[key]


def want_tree(case, wt):
    key = (case[0], "tree")
    if key not in _WANT:
        _WANT[key] = ls.expected(case[1], np.asarray(case[2], dtype=np.int64).reshape(-1, 2), weights=wt)
    return _WANT[key]


def _min_rounds(case, grid, merging):
    """(module docstring) K + 2 for a corridor, + 1 with merging; any other case: one stamp round and one label round."""
    k = t2.corridor_K(case[0], grid) if case[0].startswith("w/") else 0
    return k + 2 + int(merging)


def _on_device(case):
    import torch
    dev = torch.device("cuda", 0)
    field = torch.from_numpy(np.ascontiguousarray(case[1])).to(dev)
    s = torch.from_numpy(np.asarray(case[2], dtype=np.int64).reshape(-1, 2).astype(np.int32)).to(dev)
    return field, s


def _check_tiles(spans, want, tag):
    """The owned rectangles equal the oracle, and every tile's halo ring holds the owner's labels (the ring's four corner cells
    are nobody's stencil): as test_gpu_group._tiled2d."""
    for (r0, r1, lo, hi), (c0, c1, clo, chi), lab in spans:
        L = lab.cpu().numpy().view(np.uint32)
        assert L.shape == (hi - lo, chi - clo)
        assert (L[r0 - lo:r1 - lo, c0 - clo:c1 - clo] == want[r0:r1, c0:c1]).all(), (tag, "owned", r0, c0)
        if lo < r0:
            assert (L[0, c0 - clo:c1 - clo] == want[lo, c0:c1]).all(), (tag, "top halo", r0, c0)
        if hi > r1:
            assert (L[-1, c0 - clo:c1 - clo] == want[hi - 1, c0:c1]).all(), (tag, "bottom halo", r0, c0)
        if clo < c0:
            assert (L[r0 - lo:r1 - lo, 0] == want[r0:r1, clo]).all(), (tag, "left halo", r0, c0)
        if chi > c1:
            assert (L[r0 - lo:r1 - lo, -1] == want[r0:r1, chi - 1]).all(), (tag, "right halo", r0, c0)


# ---- host form: ws_segment_tiled2d --------------------------------------------------------------------------------------------------

@_params("tuvwxyz")
def test_host_field_in_2d_tiles_equals_the_oracle(pkg, groups, case, grid):
    name = case[0]
    py, px = grid
    g = groups[py * px]
    edge, shift = tc.edge_options(name)
    got, rounds = segment_tiled2d(pkg, g, case, py, px, edge=edge, shift=shift)
    want = want_segment(case)
    assert got.shape == want.shape and (got == want).all(), (name, grid, int((got != want).sum()))
    assert rounds >= _min_rounds(case, grid, False), (name, grid, rounds)
    for level in t2.merge_levels(name):
        got, rounds = segment_tiled2d(pkg, g, case, py, px, merging=True, max_level=level, edge=edge, shift=shift)
        want = want_merge(case, level)
        assert (got == want).all(), (name, grid, level, int((got != want).sum()))
        if level == 254:
            assert rounds >= _min_rounds(case, grid, True), (name, grid, rounds)


# ---- device form: ws_segment_tiled2d_device on the tiles of Group.make_blocks2d -----------------------------------------------------

@_params("tuvwxy")
def test_device_tiles_equal_the_oracle_and_the_halo_ring_holds_the_owners_labels(pkg, groups, case, grid):
    name, img, seeds, _ = case
    py, px = grid
    g = groups[py * px]
    H, W = img.shape
    field, s = _on_device(case)
    blocks, spans, keep = g.make_blocks2d(field, s, py, px)
    rounds = g.segment_tiled2d_device(H, W, py, px, blocks, n_seeds_total=len(seeds))
    _check_tiles(spans, want_segment(case), (name, grid, "segmenting"))
    assert rounds >= _min_rounds(case, grid, False), (name, grid, rounds)
    for level in t2.merge_levels(name):
        rounds = g.segment_tiled2d_device(H, W, py, px, blocks, max_level=level, n_seeds_total=len(seeds), merging=True)
        _check_tiles(spans, want_merge(case, level), (name, grid, level))
        if level == 254:
            assert rounds >= _min_rounds(case, grid, True), (name, grid, rounds)


# ---- lists: ws_transform_to_list_tiled2d_device -------------------------------------------------------------------------------------

LIST_PAIRS = [(c, g) for c, g in t2.pairs("vwxy") if c[0][0] != "w" or ("/spiral/" in c[0] and g == (2, 2) and c[1].size < 10000)]      # w: (ii) only


@pytest.mark.parametrize("merging", [1, 0])
@pytest.mark.parametrize("case,grid", LIST_PAIRS, ids=[t2.pair_id(c, g) for c, g in LIST_PAIRS])
def test_lists_of_a_field_in_2d_tiles_equal_the_oracle(pkg, groups, case, grid, merging):
    import torch
    name, img, seeds, _ = case
    py, px = grid
    g = groups[py * px]
    ffi = pkg._ffi
    H, W = img.shape
    field, s = _on_device(case)
    blocks, spans, keep = g.make_blocks2d(field, s, py, px)
    cap = 255 * (len(seeds) + 1)
    lakes = torch.zeros((cap, 2), dtype=torch.int64, device=field.device)
    n_lakes = ctypes.c_size_t(0)
    offsets, uncol = np.zeros(256, dtype=np.uint64), np.zeros(255, dtype=np.uint64)
    opt = ffi.Options(254)
    rc = ffi.lib().ws_transform_to_list_tiled2d_device(g._h, H, W, py, px, len(seeds), blocks, ctypes.byref(opt), int(merging), lakes.data_ptr(), cap,
                                                       ctypes.byref(n_lakes), offsets.ctypes.data, uncol.ctypes.data, None)
    assert rc == 0, (name, rc, ffi.lib().ws_group_last_error(g._h))
    check_lists(lakes.cpu().numpy().view(np.uint64), n_lakes.value, offsets, uncol, want_lists(case, merging), H * W, (name, grid, merging))
    _check_tiles(spans, want_segment(case), (name, grid, "after the lists"))      # the tiles hold the segmenting labels


# ---- tree and catalogue: ws_merge_tree_tiled2d_device -------------------------------------------------------------------------------

def _u16(shape, seed):
    """A u16 weight plane that is no function of the image and holds 0 and 65535 several times each (ties at the peak)."""
    rng = np.random.default_rng(2000 + seed)
    wt = rng.integers(0, 65536, shape, dtype=np.uint16)
    flat = wt.reshape(-1)
    where = rng.permutation(flat.size)
    flat[where[:max(flat.size // 50, 2)]] = 65535
    flat[where[-max(flat.size // 50, 2):]] = 0
    return wt


@_params("vxy")
def test_tree_and_catalogue_of_a_field_in_2d_tiles_equal_the_oracle_and_the_single_context(pkg, eng, groups, case, grid):
    import torch
    name, img, seeds, _ = case
    py, px = grid
    g = groups[py * px]
    H, W = img.shape
    wt = _u16((H, W), len(name))
    field, s = _on_device(case)
    t_wt = torch.from_numpy(wt.view(np.int16)).to(field.device)
    one_tree, one = eng.merge_tree_stats(field, s, weights=t_wt)
    blocks, spans, keep = g.make_blocks2d(field, s, py, px)
    tree, stats, _ = g.merge_tree_tiled2d_device(H, W, py, px, len(seeds), blocks, weights=t_wt, want_stats=True)
    torch.cuda.synchronize()
    tree, stats, one_tree, one = (t.cpu().numpy() for t in (tree, stats, one_tree, one))
    o_tree, o_rec = want_tree(case, wt)
    assert (tree.view(np.uint32) == o_tree).all(), (name, grid, "oracle tree")
    assert ls.mismatch(ls.from_raw(stats), o_rec) is None, (name, grid, ls.mismatch(ls.from_raw(stats), o_rec))
    assert (tree == one_tree).all(), (name, grid, "single-context tree")
    assert (stats == one).all(), (name, grid, ls.mismatch(ls.from_raw(stats), ls.from_raw(one)))
    _check_tiles(spans, want_segment(case), (name, grid, "after the tree"))
