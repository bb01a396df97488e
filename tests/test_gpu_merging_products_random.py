"""The merging transform's per-level products -- history planes, lake lists, the merge tree, the lake catalogue, and the cube form
of each -- under load, against the CPU oracle, -m gpu: the sweep and the constructed fields of tests/merging_cases.py (plateaus,
walls and floors, shuffled and duplicated seed lists, border seeds, a parent chain 254 deep, 22 k deaths at level 0, two seas
joined by one pixel) on shapes of many relaxation tiles.  ONE engine on a stream of its own serves the whole module, device and
host forms alike, so the level loops are captured and replayed across cases whose contents differ.  Every comparison is on
integers and exact; what a case reaches is proved without a GPU in tests/test_merging_cases_cpu.py."""
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import lake_stats_ref as ls
import merging_cases as mc

pytestmark = pytest.mark.gpu

HOST_HISTORY_CALL_WORDS = 1 << 24     # the host form's u64 planes: a longer level list goes in calls of at most 128 MiB each


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def eng(pkg):
    import torch
    with torch.cuda.stream(torch.cuda.Stream(0)):      # a stream of its own: the level loops are captured and replayed
        yield importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


@pytest.fixture(scope="module")
def sweep():
    return mc.sweep_cases()


@pytest.fixture(scope="module")
def constructed():
    return {c.name: c for c in mc.constructed_cases()}


@pytest.fixture(scope="module")
def cubes():
    return mc.cube_cases()


def _ws(pkg, eng, case, merging=True):
    """The host form on the engine's own context."""
    b = pkg.TransformBuilder.new().set_max_water_lvl(case.max_level).set_context(eng.ctx)
    if case.edge:
        b.enable_edge_correction()
    if case.seed_shift:
        b.shift_seeds_into_padded_plane()
    return b.build_merging() if merging else b.build_segmenting()


def _to_dev(eng, img, seeds):
    import torch
    t_img = torch.from_numpy(np.ascontiguousarray(img)).to(eng.device)
    t_seeds = torch.from_numpy(np.asarray(seeds, dtype=np.int64).reshape(-1, 2).astype(np.int32)).to(eng.device).contiguous()
    return t_img, t_seeds


def _u32(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def _plane_mismatch(got, want):
    """None, or (number of pixels, first pixels, got, want) where two planes differ."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shape", got.shape, want.shape
    bad = np.flatnonzero(got.ravel() != want.ravel())
    return None if bad.size == 0 else (bad.size, bad[:6], got.ravel()[bad[:6]], want.ravel()[bad[:6]])


def _tree_mismatch(got, want):
    """None, or (field, colours, got, want) of the first field of the tree records that differs."""
    if got.shape != want.shape:
        return "shape", got.shape, want.shape
    for k, name in enumerate(("parent", "death_level", "area", "n_leaves")):
        bad = np.flatnonzero(got[:, k] != want[:, k])
        if bad.size:
            return name, bad.size, bad[:8], got[bad[:8], k], want[bad[:8], k]
    return None


def _lakes_mismatch(colours, areas, unc, want):
    """None, or what differs between one level's records (in any order) and the oracle's (colours ascending, areas, uncoloured)."""
    cols, sizes, want_unc = want
    order = np.argsort(colours, kind="stable")
    colours, areas = np.asarray(colours)[order].astype(np.int64), np.asarray(areas)[order].astype(np.int64)
    if int(unc) != want_unc:
        return "uncoloured", int(unc), want_unc
    if colours.size != cols.size or (colours != cols).any():
        return "colours", colours.size, cols.size, np.setxor1d(colours, cols)[:8]
    bad = np.flatnonzero(areas != sizes.astype(np.int64))
    return None if bad.size == 0 else ("area", colours[bad[:8]], areas[bad[:8]], sizes[bad[:8]])


# ---- the four products of one field ----------------------------------------------------------------------------------------------

def _check_history(pkg, eng, case, e):
    """transform_history, merging and segmenting, device and host form, for the case's level list: every level of it in both
    forms.  The device form takes the list as one call; the host form, whose planes are u64, takes it in consecutive parts
    where all its planes at once would be too many.  (The device wrapper has no seed_shift: it gets the seeds in plane
    coordinates, the host form the option.)"""
    t_img, t_seeds = _to_dev(eng, case.img, e.ps)
    lv = case.levels
    for merging, want in ((True, e.planes), (False, e.seg_planes)):
        got = _u32(eng.transform_history(t_img, t_seeds, levels=lv, merging=merging, max_level=case.max_level, edge=case.edge))
        assert got.shape == (len(lv),) + case.plane_shape
        for k, L in enumerate(lv):
            assert _plane_mismatch(got[k], want[L]) is None, (case, "device", merging, L, _plane_mismatch(got[k], want[L]))
        del got
        ws = _ws(pkg, eng, case, merging)
        per_call = max(1, HOST_HISTORY_CALL_WORDS // (case.plane_shape[0] * case.plane_shape[1]))
        seen = []
        for first in range(0, len(lv), per_call):
            host = ws.transform_history_levels(case.img, case.seeds, lv[first:first + per_call])
            for (L, p) in host:
                assert _plane_mismatch(p, want[L]) is None, (case, "host", merging, L, _plane_mismatch(p, want[L]))
            seen += [l for l, _ in host]
        assert seen == lv


def _check_lists(pkg, eng, case, e, live_list):
    """transform_to_list (merging), device and host form, every level against find_lake_sizes of the oracle's plane; live_list:
    every level's records from the list of the lakes alive at the level before, whatever the number of colours."""
    import torch
    L = pkg._ffi.lib()
    t_img, t_seeds = _to_dev(eng, case.img, e.ps)
    if live_list:
        assert L.ws_ctx_set_live_list_min_colours(eng.ctx.handle, 1) == 0
    try:
        lakes, offsets, unc = eng.transform_to_list(t_img, t_seeds, merging=True, max_level=case.max_level, edge=case.edge)
        torch.cuda.synchronize()
        rec = lakes.cpu().numpy()
        host = _ws(pkg, eng, case).transform_to_list_sparse(case.img, case.seeds)
    finally:
        assert L.ws_ctx_set_live_list_min_colours(eng.ctx.handle, 0) == 0
    assert len(offsets) == case.max_level + 2 and int(offsets[-1]) == len(rec) and len(host) == case.max_level + 1
    for lvl in range(case.max_level + 1):
        r = rec[int(offsets[lvl]):int(offsets[lvl + 1])]
        bad = _lakes_mismatch(r[:, 0], r[:, 1], unc[lvl], e.lakes[lvl])
        assert bad is None, (case, "device", live_list, lvl, bad)
        hl, hunc, hcol, harea = host[lvl]
        bad = _lakes_mismatch(hcol, harea, hunc, e.lakes[lvl])
        assert hl == lvl and bad is None, (case, "host", live_list, lvl, bad)


def _check_tree(pkg, eng, case, e, replays=None):
    """merge_tree with labels, device and host form.  replays: the device call runs on buffers that held another image (this one
    mirrored) for two calls before, so that the level loop's captured graphs are replayed on contents that differ; the list
    collects the graph launches of the call that counts."""
    import torch
    t_img, t_seeds = _to_dev(eng, case.img, case.seeds)
    kw = dict(max_level=case.max_level, edge=case.edge, seed_shift=case.seed_shift, want_labels=True)
    if replays is not None:
        out = torch.empty((len(case.seeds) + 1, 4), dtype=torch.int32, device=eng.device)
        real = t_img.clone()
        t_img.copy_(torch.from_numpy(np.ascontiguousarray(case.img[:, ::-1])))
        for _ in range(2):
            eng.merge_tree(t_img, t_seeds, out=out, **kw)
        t_img.copy_(real)
        kw["out"] = out
    tree, labels = eng.merge_tree(t_img, t_seeds, **kw)
    dev, dev_labels = _u32(tree), _u32(labels)
    if replays is not None:
        replays.append(eng.stats()["graph_launches"])
    assert _tree_mismatch(dev, e.tree) is None, (case, "device", _tree_mismatch(dev, e.tree))
    assert _plane_mismatch(dev_labels, e.labels) is None, (case, "device labels", _plane_mismatch(dev_labels, e.labels))
    host = _ws(pkg, eng, case).merge_tree(case.img, case.seeds, want_labels=True)
    got = np.stack([host.parent, host.death_level, host.area, host.n_leaves], axis=1)
    assert _tree_mismatch(got, e.tree) is None, (case, "host", _tree_mismatch(got, e.tree))
    assert _plane_mismatch(host.labels, e.labels) is None, (case, "host labels")


def _check_catalogue(pkg, eng, case, e):
    """merge_tree_stats, device and host form, weighed by the image, a u8 plane and a u16 plane that repeats 0 and 65535."""
    import torch
    t_img, t_seeds = _to_dev(eng, case.img, case.seeds)
    for name, wt in e.weights:
        want = e.stats[name]
        t_wt = None if wt is None else torch.from_numpy(wt if wt.dtype == np.uint8 else wt.view(np.int16)).to(eng.device)
        tree, raw = eng.merge_tree_stats(t_img, t_seeds, weights=t_wt, max_level=case.max_level, edge=case.edge, seed_shift=case.seed_shift)
        assert _tree_mismatch(_u32(tree), e.tree) is None, (case, name, "device tree", _tree_mismatch(_u32(tree), e.tree))
        rec = ls.from_raw(raw.cpu().numpy())
        assert ls.mismatch(rec, want) is None, (case, name, "device", ls.mismatch(rec, want))
        host_tree, host = _ws(pkg, eng, case).merge_tree_stats(case.img, case.seeds, weights=wt)
        got = np.stack([host_tree.parent, host_tree.death_level, host_tree.area, host_tree.n_leaves], axis=1)
        assert _tree_mismatch(got, e.tree) is None, (case, name, "host tree", _tree_mismatch(got, e.tree))
        assert ls.mismatch(host, want) is None, (case, name, "host", ls.mismatch(host, want))
    assert (e.stats["image"]["reserved"] == 0).all()


def test_history_planes_of_the_sweep(pkg, eng, sweep):
    for case in sweep:
        _check_history(pkg, eng, case, mc.expected(case))


def test_lake_lists_of_the_sweep(pkg, eng, sweep):
    for i, case in enumerate(sweep):
        _check_lists(pkg, eng, case, mc.expected(case), live_list=i % 2 == 0)


def test_merge_trees_of_the_sweep(pkg, eng, sweep):
    replays = []
    for case in sweep:
        _check_tree(pkg, eng, case, mc.expected(case), replays)
    assert sum(r > 0 for r in replays) >= len(sweep) // 2, replays      # the level loops did run as replayed graphs


def test_lake_catalogues_of_the_sweep(pkg, eng, sweep):
    """(On the six-level fields the image weighs: almost every peak_pixel is decided by the first-in-row-major rule.)"""
    for case in sweep:
        _check_catalogue(pkg, eng, case, mc.expected(case))


def _all_products(pkg, eng, case):
    """Every product of a constructed case; its history at every level, 0 .. max_level."""
    assert case.levels == list(range(case.max_level + 1)), case
    e = mc.expected(case)
    _check_history(pkg, eng, case, e)
    _check_lists(pkg, eng, case, e, live_list=False)
    _check_lists(pkg, eng, case, e, live_list=True)
    _check_tree(pkg, eng, case, e)
    _check_catalogue(pkg, eng, case, e)
    return e


def test_staircase_chain_254_deep_every_product(pkg, eng, constructed):
    """DESIGN.md 4.1 'Not bounded': a walk as long as the chain of hooks does not change the result.  Every level's plane."""
    case = constructed["staircase"]
    e = _all_products(pkg, eng, case)
    assert mc.describe(case, e)["depth"] == 254


@pytest.mark.parametrize("w", [516, 517])
def test_seeded_plateau_mass_deaths_at_level_zero_every_product(pkg, eng, constructed, w):
    case = constructed[f"plateau_w{w}"]
    e = _all_products(pkg, eng, case)
    assert int((e.death == 0).sum()) >= 20000


def test_two_seas_merge_exactly_from_the_joining_level_on_every_product(pkg, eng, constructed):
    v = mc.TWO_SEAS_V
    for max_level in (v - 1, v, 254):
        _all_products(pkg, eng, constructed[f"two_seas_max{max_level}"])


# ---- cubes of slices -------------------------------------------------------------------------------------------------------------

def _cube_inputs(eng, slices):
    import torch
    lists = [c.seeds for c in slices]
    flat = np.concatenate(lists, axis=0) if sum(len(l) for l in lists) else np.zeros((0, 2), np.int64)
    offs = [0] + [int(x) for x in np.cumsum([len(l) for l in lists])]
    cube = torch.from_numpy(np.stack([c.img for c in slices])).to(eng.device).contiguous()
    return cube, torch.from_numpy(flat.astype(np.int32)).to(eng.device).contiguous(), offs


def _with_limit(eng, limit, fn):
    eng.ctx.set_batch_pixel_limit(limit)
    try:
        return fn()
    finally:
        eng.ctx.set_batch_pixel_limit(0)


def _cube_expected(slices):
    return [mc.expected(c, want_stats=False) for c in slices]


def test_history_cubes(eng, cubes):
    for slices, limit in cubes:
        c0 = slices[0]
        cube, seeds, offs = _cube_inputs(eng, slices)
        want = _cube_expected(slices)
        for merging in (True, False):
            got = _u32(_with_limit(eng, limit, lambda: eng.transform_history_batch(cube, seeds, offs, levels=c0.levels, merging=merging,
                                                                                   max_level=c0.max_level, edge=c0.edge)))
            assert got.shape == (len(slices), len(c0.levels)) + c0.plane_shape
            for k, (c, e) in enumerate(zip(slices, want)):
                planes = e.planes if merging else e.seg_planes
                for j, L in enumerate(c0.levels):
                    assert _plane_mismatch(got[k, j], planes[L]) is None, (c, merging, L, _plane_mismatch(got[k, j], planes[L]))
                if len(c.seeds) == 0:
                    assert not got[k].any(), c


def test_lake_list_cubes(eng, cubes):
    import torch
    for slices, limit in cubes:
        c0 = slices[0]
        cube, seeds, offs = _cube_inputs(eng, slices)
        want = _cube_expected(slices)
        lakes, offsets, unc = _with_limit(eng, limit, lambda: eng.transform_to_list_batch(cube, seeds, offs, merging=True,
                                                                                          max_level=c0.max_level, edge=c0.edge))
        torch.cuda.synchronize()
        rec = lakes.cpu().numpy()
        levels = c0.max_level + 1
        assert len(offsets) == len(slices) * levels + 1 and int(offsets[-1]) == len(rec)
        for k, (c, e) in enumerate(zip(slices, want)):
            for lvl in range(levels):
                b = k * levels + lvl
                r = rec[int(offsets[b]):int(offsets[b + 1])]
                bad = _lakes_mismatch(r[:, 0], r[:, 1], unc[b], e.lakes[lvl])
                assert bad is None, (c, lvl, bad)


def test_merge_tree_cubes(eng, cubes):
    for slices, limit in cubes:
        c0 = slices[0]
        cube, seeds, offs = _cube_inputs(eng, slices)
        want = _cube_expected(slices)
        tree, labels = _with_limit(eng, limit, lambda: eng.merge_tree_batch(cube, seeds, offs, max_level=c0.max_level, edge=c0.edge,
                                                                            want_labels=True))
        tree, labels = _u32(tree), _u32(labels)
        first = [offs[k] + k for k in range(len(slices) + 1)]          # slice k's n_k + 1 records
        assert tree.shape == (first[-1], 4)
        for k, (c, e) in enumerate(zip(slices, want)):
            got = tree[first[k]:first[k + 1]]
            assert _tree_mismatch(got, e.tree) is None, (c, _tree_mismatch(got, e.tree))
            assert _plane_mismatch(labels[k], e.labels) is None, (c, "labels", _plane_mismatch(labels[k], e.labels))
