"""merge_tree (ws_merge_tree_device, ws_merge_tree) against the tree derived from the CPU oracle's per-level planes
(tests/merge_tree_ref.py), and at size against the engine's own history planes and lake lists, -m gpu.  Every comparison is on
integers and exact."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import merge_tree_ref as mt
import oracle_lib as ol
import strided

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def eng(pkg):
    import torch
    with torch.cuda.stream(torch.cuda.Stream(0)):      # a stream of its own: the level loops are captured and replayed
        yield importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


def _ws(pkg, max_level=254, edge=False, seed_shift=False):
    b = pkg.TransformBuilder.new().set_max_water_lvl(max_level)
    if edge:
        b.enable_edge_correction()
    if seed_shift:
        b.shift_seeds_into_padded_plane()
    return b.build_merging()


def _to_dev(eng, img, seeds):
    import torch
    t_img = torch.from_numpy(np.ascontiguousarray(img)).to(eng.device)
    t_seeds = torch.from_numpy(np.asarray(seeds, dtype=np.int64).reshape(-1, 2).astype(np.int32)).to(eng.device)
    return t_img, t_seeds


def _device_tree(eng, img, seeds, want_labels=False, **kw):
    import torch
    t_img, t_seeds = _to_dev(eng, img, seeds)
    got = eng.merge_tree(t_img, t_seeds, want_labels=want_labels, **kw)
    torch.cuda.synchronize()
    tree, labels = got if want_labels else (got, None)
    rec = tree.cpu().numpy().view(np.uint32)
    return rec if not want_labels else (rec, labels.cpu().numpy().view(np.uint32))


def _check_both_forms(pkg, eng, img, seeds, max_level=254, edge=False, seed_shift=False, tag=None):
    parent, death, area, leaves, vals, ex = mt.expected_tree(img, seeds, max_level, edge, seed_shift)
    want = np.stack([parent, death, area, leaves], axis=1)
    dev, dev_labels = _device_tree(eng, img, seeds, want_labels=True, max_level=max_level, edge=edge, seed_shift=seed_shift)
    host = _ws(pkg, max_level, edge, seed_shift).merge_tree(img, seeds, want_labels=True)
    got = np.stack([host.parent, host.death_level, host.area, host.n_leaves], axis=1)
    for name, k in (("parent", 0), ("death_level", 1), ("area", 2), ("n_leaves", 3)):
        bad = np.flatnonzero(dev[:, k] != want[:, k])
        assert bad.size == 0, (tag, "device", name, bad[:8], dev[bad[:8]], want[bad[:8]])
        bad = np.flatnonzero(got[:, k] != want[:, k])
        assert bad.size == 0, (tag, "host", name, bad[:8], got[bad[:8]], want[bad[:8]])
    mt.check_invariants(dev[:, 0], dev[:, 1], dev[:, 2], dev[:, 3], vals, ex)
    # the labels are the segmenting ones: the tree's leaf colours
    seg = ol.segment(img, mt.plane_seeds(seeds, edge, seed_shift), max_level=max_level, edge=edge)
    assert (dev_labels == seg).all() and (host.labels == seg).all(), tag
    assert host.labels.dtype == np.uint64


@pytest.mark.parametrize("shape,seed,edge", [((24, 24), 1, False), ((50, 70), 2, False), ((96, 96), 3, True),
                                              ((130, 67), 4, False), ((200, 300), 5, True)])
def test_tree_equals_reference_on_random_fields(pkg, eng, shape, seed, edge):
    img = cases.field(*shape, seed)
    _check_both_forms(pkg, eng, img, ol.find_local_minima(img), edge=edge)


@pytest.mark.parametrize("maxlvl", [1, 60, 254])
def test_tree_max_water_level(pkg, eng, maxlvl):
    img = cases.smooth_field(90, 110, 8)
    _check_both_forms(pkg, eng, img, ol.find_local_minima(img), max_level=maxlvl)


def test_tree_adversarial_cases(pkg, eng):
    for name, img, seeds in cases.adversarial_cases():
        seeds = cases.seeds_or_maxima(img, seeds)
        for edge in (False, True):
            _check_both_forms(pkg, eng, img, seeds, edge=edge, tag=(name, edge))


def test_tree_seed_shift(pkg, eng):
    img = cases.field(61, 83, 9)
    seeds = ol.find_local_minima(img)
    _check_both_forms(pkg, eng, img, seeds, edge=True, seed_shift=True)
    _check_both_forms(pkg, eng, img, seeds, edge=True, seed_shift=False)


def test_no_seeds_writes_entry_zero_only(pkg, eng):
    import torch
    img = eng.random_field(40, 52, 3)
    none = torch.empty((0, 2), dtype=torch.int32, device=eng.device)
    out = torch.full((3, 4), 0x5A5A5A5A, dtype=torch.int32, device=eng.device)
    opt = eng.options()
    rc = pkg._ffi.lib().ws_merge_tree_device(eng.ctx.handle, img.data_ptr(), 40, 52, 52, None, 0, ctypes.byref(opt), out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    rec = out.cpu().numpy().view(np.uint32)
    assert rec[0].tolist() == [0, mt.ALIVE, 40 * 52, 0]
    assert (rec[1:] == 0x5A5A5A5A).all()
    host = _ws(pkg).merge_tree(img.cpu().numpy(), np.zeros((0, 2), dtype=np.uint64))
    assert (host.parent.tolist(), host.death_level.tolist(), host.area.tolist(), host.n_leaves.tolist()) == ([0], [mt.ALIVE], [40 * 52], [0])


def test_argument_checks_come_before_device_work(pkg, eng):
    import torch
    L = pkg._ffi.lib()
    img = eng.random_field(32, 32, 1)
    seeds = eng.find_local_minima(img)
    ns = seeds.shape[0]
    tree = torch.full((ns + 1, 4), 7, dtype=torch.int32, device=eng.device)
    opt = eng.options()
    BAD = pkg._ffi.WS_ERR_BAD_ARG
    h = eng.ctx.handle
    assert L.ws_merge_tree_device(h, None, 32, 32, 32, seeds.data_ptr(), ns, ctypes.byref(opt), tree.data_ptr(), None) == BAD
    assert L.ws_merge_tree_device(h, img.data_ptr(), 32, 32, 32, None, ns, ctypes.byref(opt), tree.data_ptr(), None) == BAD
    assert L.ws_merge_tree_device(h, img.data_ptr(), 32, 32, 32, seeds.data_ptr(), ns, ctypes.byref(opt), None, None) == BAD
    assert L.ws_merge_tree_device(h, img.data_ptr(), 32, 32, 32, seeds.data_ptr(), ns, None, tree.data_ptr(), None) == BAD
    assert L.ws_merge_tree_device(h, img.data_ptr(), 32, 32, 16, seeds.data_ptr(), ns, ctypes.byref(opt), tree.data_ptr(), None) == BAD
    himg = np.zeros((8, 8), dtype=np.uint8)
    hseeds = np.array([[1, 1]], dtype=np.uint64)
    htree = np.zeros((2, 4), dtype=np.uint32)
    assert L.ws_merge_tree(h, None, 8, 8, 8, hseeds.ctypes.data, 1, ctypes.byref(opt), htree.ctypes.data, None) == BAD
    assert L.ws_merge_tree(h, himg.ctypes.data, 8, 8, 8, None, 1, ctypes.byref(opt), htree.ctypes.data, None) == BAD
    assert L.ws_merge_tree(h, himg.ctypes.data, 8, 8, 8, hseeds.ctypes.data, 1, ctypes.byref(opt), None, None) == BAD
    bad = eng.options(max_level=255)
    assert L.ws_merge_tree_device(h, img.data_ptr(), 32, 32, 32, seeds.data_ptr(), ns, ctypes.byref(bad), tree.data_ptr(), None) == pkg._ffi.WS_ERR_MAX_TOO_HIGH
    bad = eng.options(max_level=0)
    assert L.ws_merge_tree(h, himg.ctypes.data, 8, 8, 8, hseeds.ctypes.data, 1, ctypes.byref(bad), htree.ctypes.data, None) == pkg._ffi.WS_ERR_MAX_TOO_LOW
    torch.cuda.synchronize()
    assert bool((tree == 7).all())
    # a transform in flight is refused
    out = torch.empty((32, 32), dtype=torch.int32, device=eng.device)
    eng.segment_begin(img, seeds, out)
    try:
        assert L.ws_merge_tree_device(h, img.data_ptr(), 32, 32, 32, seeds.data_ptr(), ns, ctypes.byref(opt), tree.data_ptr(), None) == BAD
        assert L.ws_merge_tree(h, himg.ctypes.data, 8, 8, 8, hseeds.ctypes.data, 1, ctypes.byref(opt), htree.ctypes.data, None) == BAD
    finally:
        eng.segment_end()
    torch.cuda.synchronize()
    assert bool((tree == 7).all())


def test_last_arrival_reports_the_tree_transforms_stamps(pkg, eng):
    img = cases.field(70, 90, 21)
    seeds = ol.find_local_minima(img)
    t_img, t_seeds = _to_dev(eng, img, seeds)
    eng.segment(t_img, t_seeds)
    want = eng.last_arrival().cpu().numpy()
    eng.segment(*_to_dev(eng, cases.field(70, 90, 22), seeds))
    eng.merge_tree(t_img, t_seeds)
    assert (eng.last_arrival().cpu().numpy() == want).all()


@pytest.fixture(scope="module")
def big(eng):
    """2048^2 random field: the tree, the segmenting labels, the stamps."""
    import torch
    img = eng.random_field(2048, 2048, 11)
    seeds = eng.find_local_minima(img)
    tree, labels = eng.merge_tree(img, seeds, want_labels=True)
    torch.cuda.synchronize()
    arr = eng.last_arrival().cpu().numpy().view(np.uint32)
    return img, seeds, tree.cpu().numpy().view(np.uint32), labels.cpu().numpy().view(np.uint32), arr


LEVELS_AT_SIZE = [0, 61, 122, 200, 254]


def test_at_size_invariants_and_pixel_balance(big):
    img, seeds, rec, labels, arr = big
    assert rec.shape == (seeds.shape[0] + 1, 4) and seeds.shape[0] > 100000
    mt.check_invariants(rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3])
    alive = (rec[:, 1] == mt.ALIVE) & (rec[:, 3] > 0)
    assert int(rec[alive, 2].astype(np.int64).sum()) + int(rec[0, 2]) == 2048 * 2048
    assert int(rec[alive, 3].astype(np.int64).sum()) == int((rec[:, 3] > 0).sum())      # every existing colour is a leaf of one survivor
    assert int(rec[0, 2]) == int((labels == 0).sum())


def test_at_size_roots_table_gives_the_history_planes(eng, big):
    import torch
    img, seeds, rec, labels, arr = big
    planes = eng.transform_history(img, seeds, levels=LEVELS_AT_SIZE, merging=True)
    torch.cuda.synchronize()
    planes = planes.cpu().numpy().view(np.uint32)
    for k, L in enumerate(LEVELS_AT_SIZE):
        table = mt.roots_at(rec[:, 0], rec[:, 1], L)
        assert table[0] == 0
        shown = planes[k] != 0
        assert shown.any()
        assert (table[labels][shown] == planes[k][shown]).all(), L


def test_at_size_lakes_of_the_tree_are_the_lake_lists(eng, big):
    """The lakes alive after level L and their areas, from the tree, against ws_transform_to_list_device's records of level L.
    A lake's area at L is the own counts of its subtree cut at L: the pixels whose colour the tree sends to it (roots_at(L)) and
    that have arrived by L.  A surviving lake still gains pixels after L, so the cut is taken at the pixels' arrival stamps, on
    the host.  The `area` field itself is met where it is defined: a colour that dies at L + 1 was last its own lake at L."""
    img, seeds, rec, labels, arr = big
    lakes, offsets, unc = eng.transform_to_list(img, seeds, merging=True)
    lakes = lakes.cpu().numpy()
    level_of = arr >> 24
    coloured = labels != 0
    parent, death, area = rec[:, 0], rec[:, 1], rec[:, 2]
    for L in LEVELS_AT_SIZE:
        table = mt.roots_at(parent, death, L)
        here = coloured & (level_of <= L)
        size = np.bincount(table[labels[here]], minlength=rec.shape[0])
        mine = np.flatnonzero(size)
        assert (death[mine] > L).all()      # (ALIVE is above every level)
        want = lakes[int(offsets[L]):int(offsets[L + 1])]
        order = np.argsort(want[:, 0], kind="stable")
        assert (want[order, 0] == mine).all(), L
        assert (want[order, 1] == size[mine]).all(), L
        assert int(unc[L]) == int((~here).sum())
        last = np.flatnonzero(death == L + 1) if L < 254 else np.flatnonzero((death == mt.ALIVE) & (rec[:, 3] > 0))
        assert last.size and (area[last] == size[last]).all(), L


def test_at_size_every_area_is_own_count_plus_children(big):
    """Every record's area and n_leaves at size, from its own definition as a fold: own[c], the pixels that arrive while c is the
    root of their colour, is recomputed here from the arrival stamps and the segmenting labels (the parent walk advanced level
    by level); then area[c] == own[c] + sum of its children's areas and n_leaves[c] == 1 + sum of its children's leaves.  A
    colour that dies at level 0 hands on no pixel and has area 1."""
    img, seeds, rec, labels, arr = big
    parent, death, area, leaves = (rec[:, k].astype(np.int64) for k in range(4))
    n_col = rec.shape[0]
    coloured = (labels != 0) & ((arr >> 24) != 0xFF)
    lab = labels[coloured].astype(np.int64)
    lvl = (arr[coloured] >> 24).astype(np.int64)
    order = np.argsort(lvl, kind="stable")
    lab, lvl = lab[order], lvl[order]
    first = np.searchsorted(lvl, np.arange(257))
    root = np.arange(n_col, dtype=np.int64)
    own = np.zeros(n_col, dtype=np.int64)
    for t in range(255):
        dead = np.flatnonzero(death[root] <= t)
        while dead.size:
            root[dead] = parent[root[dead]]
            dead = dead[death[root[dead]] <= t]
        own += np.bincount(root[lab[first[t]:first[t + 1]]], minlength=n_col)
    assert int(own.sum()) == int(coloured.sum()) and own[0] == 0
    dying = np.flatnonzero(death != mt.ALIVE)
    exists = leaves > 0
    at0 = death == 0
    assert (own[at0] == 0).all() and (area[at0] == 1).all() and (leaves[at0] == 1).all()
    handed = np.where(at0, 0, area)
    kids_area = np.bincount(parent[dying], weights=handed[dying], minlength=n_col).astype(np.int64)
    kids_leaves = np.bincount(parent[dying], weights=leaves[dying], minlength=n_col).astype(np.int64)
    check = exists & ~at0
    assert (area[check] == own[check] + kids_area[check]).all()
    assert (leaves[check] == 1 + kids_leaves[check]).all()
    assert (own[~exists] == 0).all() and (kids_area[~exists] == 0).all()


KINDS = [("w+1", 0, 0xFF), ("w+3", 5, 0x00), ("pitch", 64, "random"), ("2w", 1, 0xFF)]


@pytest.mark.parametrize("kind,offset,fill", KINDS)
def test_strided_and_offset_images(pkg, eng, kind, offset, fill):
    import torch
    img = cases.field(75, 101, 31)
    seeds = ol.find_local_minima(img)
    want = _device_tree(eng, img, seeds)
    rs = strided.row_stride_of(kind, 101)
    backing, off, _ = strided.embed(img, offset, rs, fill)
    t_back = torch.from_numpy(backing).to(eng.device)
    t_seeds = _to_dev(eng, img, seeds)[1]
    for edge in (False, True):
        ref = _device_tree(eng, img, seeds, edge=edge) if edge else want
        out = torch.empty((len(seeds) + 1, 4), dtype=torch.int32, device=eng.device)
        opt = eng.options(254, edge)
        rc = pkg._ffi.lib().ws_merge_tree_device(eng.ctx.handle, t_back.data_ptr() + off, 75, 101, rs, t_seeds.data_ptr(), len(seeds),
                                                  ctypes.byref(opt), out.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == 0
        assert (out.cpu().numpy().view(np.uint32) == ref).all(), (kind, edge)
        b = pkg.TransformBuilder.new()
        ws = (b.enable_edge_correction() if edge else b).build_merging()
        host = ws.merge_tree(strided.view(backing, off, 75, 101, rs), seeds)
        assert (np.stack([host.parent, host.death_level, host.area, host.n_leaves], axis=1) == ref).all(), (kind, edge)


def _by_level_and_colour(lakes, offsets):
    """The records of every level sorted by colour: within a level they come in the order the workgroups drew their tickets."""
    rec = lakes.cpu().numpy()
    level = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets.astype(np.int64)))
    return rec[np.lexsort((rec[:, 0], level))]


def test_alternating_with_history_list_and_merge_on_one_context(eng):
    import torch
    img = eng.random_field(300, 420, 5)
    seeds = eng.find_local_minima(img)
    levels = [3, 90, 254]
    tree0 = eng.merge_tree(img, seeds).clone()
    hist0 = eng.transform_history(img, seeds, levels=levels, merging=True).clone()
    lakes0, off0, unc0 = eng.transform_to_list(img, seeds, merging=True)
    lakes0 = _by_level_and_colour(lakes0, off0)
    merge0 = eng.merge(img, seeds).clone()
    for _ in range(3):
        assert torch.equal(eng.merge_tree(img, seeds), tree0)
        assert torch.equal(eng.transform_history(img, seeds, levels=levels, merging=True), hist0)
        assert torch.equal(eng.merge_tree(img, seeds), tree0)
        lakes, off, unc = eng.transform_to_list(img, seeds, merging=True)
        assert (off == off0).all() and (unc == unc0).all() and (_by_level_and_colour(lakes, off) == lakes0).all()
        assert torch.equal(eng.merge_tree(img, seeds), tree0)
        assert torch.equal(eng.merge(img, seeds), merge0)
    assert torch.equal(eng.transform_history(img, seeds, levels=levels, merging=True), hist0)


def test_repeated_call_replays_the_graph_bit_identically(eng):
    import torch
    img = eng.random_field(512, 512, 8)
    seeds = eng.find_local_minima(img)
    out = torch.empty((seeds.shape[0] + 1, 4), dtype=torch.int32, device=eng.device)
    first = eng.merge_tree(img, seeds, out=out).clone()
    for _ in range(4):
        assert torch.equal(eng.merge_tree(img, seeds, out=out), first)
    # statistics are per call: the last call replayed the level loop, one captured graph per group of 16 levels (a call that
    # repeats the previous one's shape captures at the latest on the second repetition)
    assert eng.stats()["graph_launches"] >= 16
