"""Thin planes and huge cubes on the GPU, -m gpu: planes with a side past 2^16 (tier A) and past 2^24 (tier B), and a cube of 70001
slices (tier C), every entry point that takes them, bit for bit against the expected values of tests/extreme_cases.py -- every
pixel and every record, nothing sampled.  tests/test_extreme_cases_cpu.py proves the inputs and the expected values on the CPU.

Status: every call returns WS_OK with the exact result -- any other status, WS_ERR_HIP above all, fails the test -- but one, which
must be the documented refusal: the catalogue under u16 weights on a 2^24-line plane (WS_ERR_TOO_LARGE, a ws_last_error text that
names the limit, and the same context still does a small transform afterwards).

What these sizes reach that no other test does: gridDim.y of the sweep engine's flood step (rows, or rows / 4) and of the stacked
cube's arrival count (slices) past 65535 -- both launches go in runs of GRID_Y_MAX; with 70001 in gridDim.y they were refused --,
`dims24` false in k_relax and k_relax0_tall (row * W without __umul24), and row numbers, tile counts and row * W sums past 2^24
in the seed tables, the resolve, the merge, the tree and the catalogue (sum_r, sum_wr, peak_pixel grow with the row number).

The sweep engine runs on all ten tier A shapes.  Tier B leaves out the per-level lists (3.5 M seeds x 255 levels) and the minima
entry points: k_minima_write sums all earlier strips in every workgroup, quadratic in H (at 262153 rows the whole
find_local_minima call, both passes and the count's copy back, took 1.30 ms; test_tier_a_minima prints it).

Wall times on an MI355X (s, the oracle's share included; the first test of a shape pays for its expected values):
  tier A   segment (fused) and stamps: 2.8 at 262153 x 5 and 5 x 262153 (the oracle's merging run with its 255 planes), 1.2 at
           70001 x 8 and 8 x 70001, 0.3 at 3 wide, below 0.1 at 1 and 2 wide; edge correction 1.7 / 0.7 / 0.2 / 0.1 (two oracle
           runs); tiled 1.1 (70001 x 8: four group calls); lists 0.3 / 0.2; every other tier A test below 0.2
  tier C   tree and catalogue 0.5, lists 0.2 each, the others below 0.1; setup (17 oracle runs) 0.02
  tier B   per shape: setup (eight oracle runs, inputs laid out) 0.3, segment and stamps 0.4 - 0.5 each mode, merge 0.3,
           history 1.0 - 1.3 (four 67 M-pixel planes stitched and compared), tree / catalogue / tree from arrival 0.5 - 1.1
"""
import ctypes
import importlib
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import extreme_cases as xc
import lake_stats_ref as ls
import oracle_lib as ol

pytestmark = pytest.mark.gpu

def _id(shape):
    return "x".join(str(s) for s in shape)


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def eng(pkg):
    import torch
    with torch.cuda.stream(torch.cuda.Stream(0)):
        yield importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


_TIER_A = {}


def tier_a(shape):
    """Image, seeds, u16 weights and the oracle's products of a tier A shape, once per module."""
    if shape not in _TIER_A:
        img, seeds = xc.tier_a_input(shape)
        wt = xc.weights_u16(shape, 1)
        _TIER_A[shape] = (img, seeds, wt, xc.products(img, seeds, levels=xc.TIER_A_LEVELS, weights=wt))
    return _TIER_A[shape]


@pytest.fixture(scope="module", params=xc.TIER_B, ids=_id)
def ch(request):
    """One chain at a time (a 2^24-line plane's inputs are 200 MB): pytest runs all tests of one shape, then the next shape's."""
    return xc.Chain(request.param)


@pytest.fixture(scope="module")
def cube():
    return xc.Cube()


def _dev(eng, img, seeds):
    import torch
    t_img = torch.from_numpy(np.ascontiguousarray(img)).to(eng.device)
    t_seeds = torch.from_numpy(np.asarray(seeds, dtype=np.int64).reshape(-1, 2).astype(np.int32)).to(eng.device).contiguous()
    return t_img, t_seeds


def _u16(eng, wt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(wt).view(np.int16)).to(eng.device)


def _u32(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def _small_transform_still_right(pkg, eng):
    img = ol.random_field(40, 52, 5)
    seeds = ol.find_local_minima(img).astype(np.int64)
    t_img, t_seeds = _dev(eng, img, seeds)
    assert (_u32(eng.segment(t_img, t_seeds)) == ol.segment_arrival(img, seeds)).all()


def call(pkg, eng, fn):
    """fn()'s result.  Every call of this module but one is known to be within the engine's limits and must return WS_OK; a
    WatershedError fails the test with its status and the ws_last_error text (WS_ERR_HIP: a launch the runtime refused)."""
    api = importlib.import_module("rustronomy_watershed_amd.api")
    try:
        return fn()
    except api.WatershedError as e:
        pytest.fail(f"status {e.status}: {e}")


def refusal(pkg, eng, fn, status):
    """fn() must be the documented refusal `status`, with a ws_last_error text that names the limit, and leave the context usable."""
    api = importlib.import_module("rustronomy_watershed_amd.api")
    with pytest.raises(api.WatershedError) as e:
        fn()
    text = pkg._ffi.lib().ws_last_error(eng.ctx.handle).decode()
    assert e.value.status == status and any(ch.isdigit() for ch in text), (e.value.status, text)
    _small_transform_still_right(pkg, eng)


def same(got, want, *tag):
    """Two planes (or record arrays) are equal everywhere."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, (tag, bad.size, bad[:6], got.ravel()[bad[:6]], want.ravel()[bad[:6]])


def same_lists(rec, offsets, unc, lakes, *tag):
    """Per level: the (colour, area) records as a sorted set, and the uncoloured count."""
    assert len(offsets) == len(lakes) + 1 and int(offsets[-1]) == len(rec), tag
    for lvl, (cols, areas, want_unc) in enumerate(lakes):
        r = rec[int(offsets[lvl]):int(offsets[lvl + 1])]
        by = np.argsort(r[:, 0], kind="stable")
        assert int(unc[lvl]) == want_unc, (tag, lvl, int(unc[lvl]), want_unc)
        assert len(r) == len(cols) and (r[by, 0] == cols).all() and (r[by, 1] == areas).all(), (tag, lvl)


# ---- tier A: a side past 2^16 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", xc.TIER_A, ids=_id)
def test_tier_a_segment_fused_and_its_stamps(pkg, eng, shape):
    img, seeds, _, p = tier_a(shape)
    t_img, t_seeds = _dev(eng, img, seeds)
    got = call(pkg, eng, lambda: eng.segment(t_img, t_seeds, engine=pkg.ENGINE_FUSED))
    same(_u32(got), p.labels, "labels")
    assert xc.stamps_mismatch(_u32(eng.last_arrival()), p.stamps) is None, xc.stamps_mismatch(_u32(eng.last_arrival()), p.stamps)


@pytest.mark.parametrize("shape", xc.TIER_A, ids=_id)
def test_tier_a_segment_sweep(pkg, eng, shape):
    """gridDim.y = rows (vector form: W % 4 == 0) or (rows + 3) / 4 (scalar form): 70001 and 65539 of them on the tall planes."""
    img, seeds, _, p = tier_a(shape)
    t_img, t_seeds = _dev(eng, img, seeds)
    got = call(pkg, eng, lambda: eng.segment(t_img, t_seeds, engine=pkg.ENGINE_SWEEP))
    same(_u32(got), p.labels, "labels")


@pytest.mark.parametrize("shape", xc.TIER_A, ids=_id)
def test_tier_a_merge(pkg, eng, shape):
    img, seeds, _, p = tier_a(shape)
    t_img, t_seeds = _dev(eng, img, seeds)
    got = call(pkg, eng, lambda: eng.merge(t_img, t_seeds))
    same(_u32(got), p.final, "final")


@pytest.mark.parametrize("shape", xc.TIER_A, ids=_id)
def test_tier_a_lists(pkg, eng, shape):
    import torch
    img, seeds, _, p = tier_a(shape)
    t_img, t_seeds = _dev(eng, img, seeds)
    for merging, lakes in ((True, p.lakes), (False, p.seg_lakes)):
        got = call(pkg, eng, lambda: eng.transform_to_list(t_img, t_seeds, merging=merging))
        rec, offsets, unc = got
        torch.cuda.synchronize()
        same_lists(rec.cpu().numpy(), offsets, unc, lakes, merging)


@pytest.mark.parametrize("shape", xc.TIER_A, ids=_id)
def test_tier_a_history(pkg, eng, shape):
    img, seeds, _, p = tier_a(shape)
    t_img, t_seeds = _dev(eng, img, seeds)
    for merging, planes in ((True, p.planes), (False, p.seg_planes)):
        got = call(pkg, eng, lambda: eng.transform_history(t_img, t_seeds, levels=xc.TIER_A_LEVELS, merging=merging))
        got = _u32(got)
        for k, L in enumerate(xc.TIER_A_LEVELS):
            same(got[k], planes[L], merging, L)


@pytest.mark.parametrize("shape", xc.TIER_A, ids=_id)
def test_tier_a_tree_and_catalogue(pkg, eng, shape):
    img, seeds, wt, p = tier_a(shape)
    t_img, t_seeds = _dev(eng, img, seeds)
    got = call(pkg, eng, lambda: eng.merge_tree_stats(t_img, t_seeds, weights=_u16(eng, wt), want_labels=True))
    tree, raw, labels = got
    same(_u32(tree), p.tree, "tree")
    same(_u32(labels), p.labels, "labels")
    rec = ls.from_raw(raw.cpu().numpy())
    assert ls.mismatch(rec, p.stats) is None, ls.mismatch(rec, p.stats)


@pytest.mark.parametrize("shape", xc.TIER_A, ids=_id)
def test_tier_a_minima(pkg, eng, shape):
    """find_local_minima and segment_minima against the oracle's list (empty on planes without an interior).  The whole
    find_local_minima call (count pass, k_minima_write, the count's copy back) took 1.30 ms at 262153 x 5, 0.61 ms at 70001 x 8."""
    import torch
    img, _, _, _ = tier_a(shape)
    want = ol.find_local_minima(img).astype(np.int64)
    t_img, _ = _dev(eng, img, want)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = call(pkg, eng, lambda: eng.find_local_minima(t_img))
    torch.cuda.synchronize()
    print(f"find_local_minima {_id(shape)}: {(time.perf_counter() - t0) * 1e3:.2f} ms")
    same(got.cpu().numpy(), want, "minima")
    got = call(pkg, eng, lambda: eng.segment_minima(t_img, want_seeds=True))
    labels, n, seeds = got
    assert n == len(want)
    same(seeds.cpu().numpy(), want, "seeds")
    same(_u32(labels), ol.segment_arrival(img, want), "labels")


@pytest.mark.parametrize("shape", xc.TIER_A, ids=_id)
def test_tier_a_edge_correction(pkg, eng, shape):
    """Inside the ring of zeros the planes of one and two lines have an interior."""
    img, seeds, _, _ = tier_a(shape)
    t_img, t_seeds = _dev(eng, img, seeds)
    got = call(pkg, eng, lambda: eng.segment(t_img, t_seeds, edge=True))
    want = ol.segment_arrival(img, seeds, edge=True)
    assert np.count_nonzero(want) > len(seeds)
    same(_u32(got), want, "segment")
    got = call(pkg, eng, lambda: eng.merge(t_img, t_seeds, edge=True))
    same(_u32(got), ol.merge_arrival(img, seeds, edge=True), "merge")


@pytest.mark.parametrize("shape", [(70001, 8), (8, 70001)], ids=_id)
def test_tier_a_host_forms(pkg, eng, shape):
    img, seeds, _, p = tier_a(shape)
    ws = pkg.TransformBuilder.new().set_context(eng.ctx).build_segmenting()
    got = call(pkg, eng, lambda: ws.transform(img, seeds))
    assert got.dtype == np.uint64
    same(got, p.labels, "ws_segment")
    for merging, lakes in ((True, p.lakes), (False, p.seg_lakes)):
        b = pkg.TransformBuilder.new().set_context(eng.ctx)
        host = call(pkg, eng, lambda: (b.build_merging() if merging else b.build_segmenting()).transform_to_list_sparse(img, seeds))
        assert len(host) == 255
        for (lvl, unc, cols, areas), (wc, wa, wu) in zip(host, lakes):
            by = np.argsort(cols, kind="stable")
            assert unc == wu and len(cols) == len(wc) and (cols[by] == wc).all() and (areas[by] == wa).all(), (merging, lvl)


@pytest.fixture(scope="module")
def groups(pkg):
    grp_mod = importlib.import_module("rustronomy_watershed_amd.group")
    gs = {world: grp_mod.Group.local(world) for world in (2, 3)}
    yield gs
    for g in gs.values():
        g.close()


def _tiled(pkg, g, img, seeds, grid=None):
    """ws_segment_tiled (grid None) or ws_segment_tiled2d at grid = (py, px): the u64 labels."""
    f = pkg._ffi
    s = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1, 2))
    img = np.ascontiguousarray(img)
    h, w = img.shape
    out = np.full((h, w), 7, dtype=np.uint64)
    opt = f.Options(254, 0, 0, 0, 0)
    rounds = ctypes.c_uint32(0)
    if grid is None:
        rc = f.lib().ws_segment_tiled(g._h, img.ctypes.data, h, w, w, s.ctypes.data, len(s), ctypes.byref(opt), 0, out.ctypes.data, ctypes.byref(rounds))
    else:
        rc = f.lib().ws_segment_tiled2d(g._h, img.ctypes.data, h, w, w, s.ctypes.data, len(s), ctypes.byref(opt), grid[0], grid[1], 0, out.ctypes.data,
                                        ctypes.byref(rounds))
    text = f.lib().ws_group_last_error(g._h)
    assert rc == f.WS_OK, (rc, text)
    return out


@pytest.mark.parametrize("shape", [(70001, 8), (8, 70001)], ids=_id)
def test_tier_a_tiled(pkg, groups, shape):
    """Row blocks on local groups of 2 and 3 ranks, and 3 x 1 and 1 x 3 tiles on the group of 3."""
    img, seeds, _, p = tier_a(shape)
    for g, grid in ((groups[2], None), (groups[3], None), (groups[3], (3, 1)), (groups[3], (1, 3))):
        got = _tiled(pkg, g, img, seeds, grid)
        same(got, p.labels, grid)


# ---- tier C: more than 2^16 slices ------------------------------------------------------------------------------------------------

def _cube_dev(eng, cube):
    import torch
    t_cube = torch.from_numpy(cube.cube).to(eng.device).contiguous()
    t_seeds = torch.from_numpy(cube.seeds.astype(np.int32)).to(eng.device).contiguous()
    return t_cube, t_seeds, [int(x) for x in cube.offsets]


def test_tier_c_segment_and_merge_batch(pkg, eng, cube):
    t_cube, t_seeds, offs = _cube_dev(eng, cube)
    got = call(pkg, eng, lambda: eng.segment_batch(t_cube, t_seeds, offs, max_level=cube.max_level))
    same(_u32(got), cube.planes(lambda p: p.labels), "segment")
    got = call(pkg, eng, lambda: eng.merge_batch(t_cube, t_seeds, offs, max_level=cube.max_level))
    same(_u32(got), cube.planes(lambda p: p.final), "merge")


@pytest.mark.parametrize("merging", [True, False], ids=["merging", "segmenting"])
def test_tier_c_lists_batch(pkg, eng, cube, merging):
    """70001 x 16 bins: the bins' sizes, the uncoloured counts, and every record -- inside a bin in any order."""
    import torch
    t_cube, t_seeds, offs = _cube_dev(eng, cube)
    got = call(pkg, eng, lambda: eng.transform_to_list_batch(t_cube, t_seeds, offs, merging=merging, max_level=cube.max_level))
    lakes, offsets, unc = got
    torch.cuda.synchronize()
    rec = lakes.cpu().numpy()
    counts, want, want_unc = cube.lists(merging)
    same(np.diff(offsets.astype(np.int64)), counts, "bin sizes")
    same(unc.astype(np.int64), want_unc, "uncoloured")
    bins = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    by = np.argsort(bins * 64 + rec[:, 0], kind="stable")          # colours stay below 64 in every slice
    assert int(cube.n_seeds_of.max()) < 64
    same(rec[by], want, "records")


def test_tier_c_history_batch(pkg, eng, cube):
    t_cube, t_seeds, offs = _cube_dev(eng, cube)
    for merging in (True, False):
        got = call(pkg, eng, lambda: eng.transform_history_batch(t_cube, t_seeds, offs, levels=cube.levels, merging=merging, max_level=cube.max_level))
        got = _u32(got)
        for j, L in enumerate(cube.levels):
            same(got[:, j], cube.planes(lambda p: (p.planes if merging else p.seg_planes)[L]), merging, L)


def test_tier_c_tree_and_catalogue_batch(pkg, eng, cube):
    t_cube, t_seeds, offs = _cube_dev(eng, cube)
    want_tree = cube.records(lambda p: p.tree)
    got = call(pkg, eng, lambda: eng.merge_tree_batch(t_cube, t_seeds, offs, max_level=cube.max_level, want_labels=True))
    same(_u32(got[0]), want_tree, "tree")
    same(_u32(got[1]), cube.planes(lambda p: p.labels), "labels")
    import torch
    t_wt = torch.from_numpy(cube.weights.view(np.int16)).to(eng.device)
    got = call(pkg, eng, lambda: eng.merge_tree_stats_batch(t_cube, t_seeds, offs, weights=t_wt, max_level=cube.max_level))
    same(_u32(got[0]), want_tree, "tree of the catalogue")
    rec, want = ls.from_raw(got[1].cpu().numpy()), cube.records(lambda p: p.stats)
    assert ls.mismatch(rec, want) is None, ls.mismatch(rec, want)


def test_tier_c_host_merge_tree_batch(pkg, eng, cube):
    """ws_merge_tree_batch: the cube, the seed lists and the records cross the bus."""
    f = pkg._ffi
    n = cube.n
    flat = np.ascontiguousarray(cube.seeds.astype(np.uint64))
    offs = np.ascontiguousarray(cube.offsets.astype(np.uintp))
    cap = int(offs[n]) + n
    tree = np.empty((cap, 4), dtype=np.uint32)
    counts = np.zeros(n, dtype=np.uintp)
    total, failed = ctypes.c_size_t(0), ctypes.c_size_t(0)
    opt = f.Options(cube.max_level, 0, 0, 0, 0)
    got = call(pkg, eng, lambda: eng.ctx.check(f.lib().ws_merge_tree_batch(eng.ctx.handle, cube.cube.ctypes.data, n, cube.h, cube.w, cube.w, cube.h * cube.w,
                                                                           flat.ctypes.data, offs.ctypes.data_as(f.szp), ctypes.byref(opt), tree.ctypes.data, cap,
                                                                           ctypes.byref(total), None, counts.ctypes.data_as(f.szp), ctypes.byref(failed))))
    assert total.value == cap
    same(tree, cube.records(lambda p: p.tree), "tree")


# ---- tier B: a side past 2^24 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("persistent", [0, 3], ids=["passes", "default"])
def test_tier_b_segment_and_its_stamps(pkg, eng, ch, persistent):
    """dims24 is false in k_relax and k_relax0_tall; 3 (the default) and 0 of ws_ctx_set_persistent_pass."""
    t_img, t_seeds = _dev(eng, ch.img, ch.seeds)
    set_mode = pkg._ffi.lib().ws_ctx_set_persistent_pass
    assert set_mode(eng.ctx.handle, persistent) == 0
    try:
        got = call(pkg, eng, lambda: eng.segment(t_img, t_seeds))
    finally:
        assert set_mode(eng.ctx.handle, 3) == 0
    same(_u32(got), ch.labels(), "labels")
    bad = xc.stamps_mismatch(_u32(eng.last_arrival()), ch.stamps())
    assert bad is None, bad


def test_tier_b_merge(pkg, eng, ch):
    t_img, t_seeds = _dev(eng, ch.img, ch.seeds)
    got = call(pkg, eng, lambda: eng.merge(t_img, t_seeds))
    same(_u32(got), ch.final(), "final")


def test_tier_b_history(pkg, eng, ch):
    t_img, t_seeds = _dev(eng, ch.img, ch.seeds)
    for merging in (True, False):
        got = call(pkg, eng, lambda: eng.transform_history(t_img, t_seeds, levels=xc.TIER_B_LEVELS, merging=merging))
        got = _u32(got)
        for k, L in enumerate(xc.TIER_B_LEVELS):
            same(got[k], ch.plane(L, merging), merging, L)


def test_tier_b_tree_catalogue_and_tree_from_arrival(pkg, eng, ch):
    """ws_merge_tree_device, ws_merge_tree_stats_device (sum_r, sum_wr and peak_pixel carry the row number) and
    ws_merge_tree_from_arrival_device on the stamps and labels of the catalogue's own flood.  With u16 weights 65535 * pixels *
    lines passes 2^64 on these planes: the documented WS_ERR_TOO_LARGE of ws_merge_tree_stats_device, and the call must be that
    refusal; u8 weights reach the kernels."""
    import torch
    t_img, t_seeds = _dev(eng, ch.img, ch.seeds)
    want_tree = ch.tree()
    got = call(pkg, eng, lambda: eng.merge_tree(t_img, t_seeds))
    same(_u32(got), want_tree, "merge_tree")
    assert 65535 * ch.img.size * max(ch.shape) >= 1 << 64 > 255 * ch.img.size * max(ch.shape)
    t_wt = _u16(eng, ch.weights)
    refusal(pkg, eng, lambda: eng.merge_tree_stats(t_img, t_seeds, weights=t_wt), pkg._ffi.WS_ERR_TOO_LARGE)
    del t_wt
    t_wt = torch.from_numpy(ch.weights8).to(eng.device)
    got = call(pkg, eng, lambda: eng.merge_tree_stats(t_img, t_seeds, weights=t_wt, want_labels=True))
    tree, raw, labels = got
    same(_u32(tree), want_tree, "merge_tree_stats")
    want = ch.stats(u8=True)
    rec = ls.from_raw(raw.cpu().numpy())
    assert ls.mismatch(rec, want) is None, ls.mismatch(rec, want)
    keys = eng.last_arrival()
    got = call(pkg, eng, lambda: eng.merge_tree_from_arrival(keys, labels, ch.n_seeds, weights=t_wt, want_stats=True))
    same(_u32(got[0]), want_tree, "from arrival")
    rec = ls.from_raw(got[1].cpu().numpy())
    assert ls.mismatch(rec, want) is None, ls.mismatch(rec, want)
