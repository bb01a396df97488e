"""merge_tree_stats (ws_merge_tree_stats_device, ws_merge_tree_stats) against the records derived from the CPU oracle's per-level
planes (tests/lake_stats_ref.py), and at size against the engine's own stamps, labels and history planes, -m gpu.  Every
comparison is on integers and exact."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import lake_stats_ref as ls
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


def _weights_to_dev(eng, wt):
    """A u8 plane as it is, a u16 plane as its int16 bits."""
    import torch
    if wt is None:
        return None
    wt = np.ascontiguousarray(wt)
    return torch.from_numpy(wt if wt.dtype == np.uint8 else wt.view(np.int16)).to(eng.device)


def _weight_planes(shape, seed):
    """The three weight choices: none (the image: many ties, so the first-in-row-major rule of peak_pixel is exercised), a u8
    plane, and a u16 plane that uses 0 and 65535 -- each several times, so the peak has ties there too -- neither a function of
    the image."""
    rng = np.random.default_rng(1000 + seed)
    u8 = rng.integers(0, 256, shape, dtype=np.uint8)
    u16 = rng.integers(0, 65536, shape, dtype=np.uint16)
    flat = u16.reshape(-1)
    where = rng.permutation(flat.size)
    flat[where[:max(flat.size // 50, 2)]] = 65535
    flat[where[-max(flat.size // 50, 2):]] = 0
    return [("image", None), ("u8", u8), ("u16", u16)]


def _device_stats(eng, img, seeds, wt, **kw):
    import torch
    t_img, t_seeds = _to_dev(eng, img, seeds)
    tree, raw = eng.merge_tree_stats(t_img, t_seeds, weights=_weights_to_dev(eng, wt), **kw)
    torch.cuda.synchronize()
    return tree.cpu().numpy().view(np.uint32), ls.from_raw(raw.cpu().numpy())


def _check_both_forms(pkg, eng, img, seeds, max_level=254, edge=False, seed_shift=False, tag=None, weights=None):
    import torch
    img = np.ascontiguousarray(img)
    planes, ps = mt.oracle_planes(img, seeds, max_level, edge, seed_shift)
    parent, death, area, leaves, vals, ex = mt.tree_from_planes(planes, ps)
    want_tree = np.stack([parent, death, area, leaves], axis=1)
    # the returned tree is what merge_tree returns for the same call
    t_img, t_seeds = _to_dev(eng, img, seeds)
    plain = eng.merge_tree(t_img, t_seeds, max_level=max_level, edge=edge, seed_shift=seed_shift)
    torch.cuda.synchronize()
    plain = plain.cpu().numpy().view(np.uint32)
    assert (plain == want_tree).all(), tag
    for name, wt in (weights if weights is not None else _weight_planes(img.shape, 0)):
        want = ls.stats_from_planes(planes, ps, ls.plane_weights(img, wt, edge), death, ex)
        tree, rec = _device_stats(eng, img, seeds, wt, max_level=max_level, edge=edge, seed_shift=seed_shift)
        assert (tree == plain).all(), (tag, name, "device tree")
        assert ls.mismatch(rec, want) is None, (tag, name, "device", ls.mismatch(rec, want))
        host_tree, host = _ws(pkg, max_level, edge, seed_shift).merge_tree_stats(img, seeds, weights=wt)
        got = np.stack([host_tree.parent, host_tree.death_level, host_tree.area, host_tree.n_leaves], axis=1)
        assert (got == plain).all(), (tag, name, "host tree")
        assert host.dtype == pkg.api.LAKE_STATS_DTYPE
        assert ls.mismatch(host, want) is None, (tag, name, "host", ls.mismatch(host, want))
        assert (want["reserved"] == 0).all()


@pytest.mark.parametrize("shape,seed,edge", [((24, 24), 1, False), ((50, 70), 2, False), ((96, 96), 3, True),
                                              ((130, 67), 4, False), ((200, 300), 5, True)])
def test_stats_equal_reference_on_random_fields(pkg, eng, shape, seed, edge):
    img = cases.field(*shape, seed)
    _check_both_forms(pkg, eng, img, ol.find_local_minima(img), edge=edge, weights=_weight_planes(shape, seed))


@pytest.mark.parametrize("maxlvl", [1, 60, 254])
def test_stats_max_water_level(pkg, eng, maxlvl):
    img = cases.smooth_field(90, 110, 8)
    _check_both_forms(pkg, eng, img, ol.find_local_minima(img), max_level=maxlvl, weights=_weight_planes(img.shape, 8))


def test_stats_adversarial_cases(pkg, eng):
    for name, img, seeds in cases.adversarial_cases():
        seeds = cases.seeds_or_maxima(img, seeds)
        for edge in (False, True):
            _check_both_forms(pkg, eng, img, seeds, edge=edge, tag=(name, edge), weights=_weight_planes(np.asarray(img).shape, 17))


def test_stats_seed_shift(pkg, eng):
    img = cases.field(61, 83, 9)
    seeds = ol.find_local_minima(img)
    _check_both_forms(pkg, eng, img, seeds, edge=True, seed_shift=True, weights=_weight_planes(img.shape, 9))
    _check_both_forms(pkg, eng, img, seeds, edge=True, seed_shift=False, weights=_weight_planes(img.shape, 9))


KINDS = [("w+1", 0, 0xFF), ("w+3", 5, 0x00), ("pitch", 64, "random"), ("2w", 1, 0xFF)]


@pytest.mark.parametrize("kind,offset,fill", KINDS)
def test_strided_and_offset_images_and_weights(pkg, eng, kind, offset, fill):
    """Image and weight plane both strided and offset, with different strides: the weights' is the image's plus 3 elements."""
    import torch
    h, w = 75, 101
    img = cases.field(h, w, 31)
    seeds = ol.find_local_minima(img)
    t_seeds = _to_dev(eng, img, seeds)[1]
    rs = strided.row_stride_of(kind, w)
    backing, off, _ = strided.embed(img, offset, rs, fill)
    t_back = torch.from_numpy(backing).to(eng.device)
    ws_rs = rs + 3
    for name, wt in _weight_planes((h, w), 31)[1:]:
        item = wt.dtype.itemsize
        wback = np.random.default_rng(5).integers(0, 256, (16 + offset + h * ws_rs) * item, dtype=np.uint8).view(wt.dtype)
        woff = 8 + offset
        wview = np.lib.stride_tricks.as_strided(wback[woff:], shape=(h, w), strides=(ws_rs * item, item))
        wview[...] = wt
        t_wback = torch.from_numpy(wback.view(np.uint8)).to(eng.device)
        for edge in (False, True):
            ref_tree, ref = _device_stats(eng, img, seeds, wt, edge=edge)
            tree = torch.empty((len(seeds) + 1, 4), dtype=torch.int32, device=eng.device)
            raw = torch.empty((len(seeds) + 1, 9), dtype=torch.int64, device=eng.device)
            opt = eng.options(254, edge)
            rc = pkg._ffi.lib().ws_merge_tree_stats_device(eng.ctx.handle, t_back.data_ptr() + off, h, w, rs, t_seeds.data_ptr(), len(seeds),
                                                            ctypes.byref(opt), t_wback.data_ptr() + woff * item,
                                                            pkg._ffi.WS_DTYPES[wt.dtype.name], ws_rs, tree.data_ptr(), raw.data_ptr(), None)
            torch.cuda.synchronize()
            assert rc == 0
            assert (tree.cpu().numpy().view(np.uint32) == ref_tree).all(), (kind, name, edge)
            assert ls.mismatch(ls.from_raw(raw.cpu().numpy()), ref) is None, (kind, name, edge)
            host_tree, host = _ws(pkg, 254, edge).merge_tree_stats(strided.view(backing, off, h, w, rs), seeds, weights=wview)
            assert (host_tree.area == ref_tree[:, 2]).all() and ls.mismatch(host, ref) is None, (kind, name, edge)
    # no weight plane: the strided image weighs
    ref_tree, ref = _device_stats(eng, img, seeds, None)
    raw = torch.empty((len(seeds) + 1, 9), dtype=torch.int64, device=eng.device)
    tree = torch.empty((len(seeds) + 1, 4), dtype=torch.int32, device=eng.device)
    opt = eng.options()
    rc = pkg._ffi.lib().ws_merge_tree_stats_device(eng.ctx.handle, t_back.data_ptr() + off, h, w, rs, t_seeds.data_ptr(), len(seeds),
                                                    ctypes.byref(opt), None, 99, 0, tree.data_ptr(), raw.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and ls.mismatch(ls.from_raw(raw.cpu().numpy()), ref) is None
    host = _ws(pkg).merge_tree_stats(strided.view(backing, off, h, w, rs), seeds)[1]
    assert ls.mismatch(host, ref) is None


def test_no_seeds_writes_entry_zero_only(pkg, eng):
    import torch
    img = eng.random_field(40, 52, 3)
    himg = img.cpu().numpy()
    tree = torch.full((3, 4), 0x5A5A5A5A, dtype=torch.int32, device=eng.device)
    raw = torch.full((3, 9), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=eng.device)
    opt = eng.options()
    rc = pkg._ffi.lib().ws_merge_tree_stats_device(eng.ctx.handle, img.data_ptr(), 40, 52, 52, None, 0, ctypes.byref(opt), None, 0, 0,
                                                    tree.data_ptr(), raw.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    whole = ls.records_by_label(np.zeros((40, 52), dtype=np.int64), himg, 1)[0]
    assert tree.cpu().numpy().view(np.uint32)[0].tolist() == [0, mt.ALIVE, 40 * 52, 0]
    assert bool((tree[1:] == 0x5A5A5A5A).all()) and bool((raw[1:] == 0x5A5A5A5A5A5A5A5A).all())
    assert ls.from_raw(raw.cpu().numpy())[0] == whole
    assert int(whole["sum_r"]) == 52 * (39 * 40 // 2) and int(whole["peak_pixel"]) == int(np.argmax(himg))
    host_tree, host = _ws(pkg).merge_tree_stats(himg, np.zeros((0, 2), dtype=np.uint64))
    assert host.shape == (1,) and host[0] == whole and host_tree.area.tolist() == [40 * 52]


def test_argument_checks_come_before_device_work(pkg, eng):
    import torch
    L = pkg._ffi.lib()
    F = pkg._ffi
    img = eng.random_field(32, 32, 1)
    seeds = eng.find_local_minima(img)
    ns = seeds.shape[0]
    tree = torch.full((ns + 1, 4), 7, dtype=torch.int32, device=eng.device)
    raw = torch.full((ns + 1, 9), 7, dtype=torch.int64, device=eng.device)
    wt = torch.zeros((32, 32), dtype=torch.int16, device=eng.device)
    opt = eng.options()
    o = ctypes.byref(opt)
    h = eng.ctx.handle
    U16, U8 = F.WS_DTYPES["uint16"], F.WS_DTYPES["uint8"]
    dev = L.ws_merge_tree_stats_device
    i, s, t, r, w = img.data_ptr(), seeds.data_ptr(), tree.data_ptr(), raw.data_ptr(), wt.data_ptr()
    assert dev(h, None, 32, 32, 32, s, ns, o, w, U16, 32, t, r, None) == F.WS_ERR_BAD_ARG
    assert dev(h, i, 32, 32, 32, None, ns, o, w, U16, 32, t, r, None) == F.WS_ERR_BAD_ARG
    assert dev(h, i, 32, 32, 32, s, ns, o, w, U16, 32, None, r, None) == F.WS_ERR_BAD_ARG
    assert dev(h, i, 32, 32, 32, s, ns, o, w, U16, 32, t, None, None) == F.WS_ERR_BAD_ARG
    assert dev(h, i, 32, 32, 32, s, ns, None, w, U16, 32, t, r, None) == F.WS_ERR_BAD_ARG
    assert dev(h, i, 32, 32, 16, s, ns, o, w, U16, 32, t, r, None) == F.WS_ERR_BAD_ARG          # a short image stride
    assert dev(h, i, 32, 32, 32, s, ns, o, w, U16, 31, t, r, None) == F.WS_ERR_BAD_ARG          # a short weight stride
    for bad_dtype in (F.WS_DTYPES["float32"], F.WS_DTYPES["int16"], F.WS_DTYPES["int32"], 17, -1):
        assert dev(h, i, 32, 32, 32, s, ns, o, w, bad_dtype, 32, t, r, None) == F.WS_ERR_UNSUPPORTED
    himg = np.zeros((8, 8), dtype=np.uint8)
    hseeds = np.array([[1, 1]], dtype=np.uint64)
    htree = np.full((2, 4), 9, dtype=np.uint32)
    hrec = np.full(2 * 9, 9, dtype=np.uint64)
    hw = np.zeros((8, 8), dtype=np.uint8)
    host = L.ws_merge_tree_stats
    a = (himg.ctypes.data, hseeds.ctypes.data, htree.ctypes.data, hrec.ctypes.data, hw.ctypes.data)
    assert host(h, None, 8, 8, 8, a[1], 1, o, a[4], U8, 8, a[2], a[3], None) == F.WS_ERR_BAD_ARG
    assert host(h, a[0], 8, 8, 8, None, 1, o, a[4], U8, 8, a[2], a[3], None) == F.WS_ERR_BAD_ARG
    assert host(h, a[0], 8, 8, 8, a[1], 1, o, a[4], U8, 8, None, a[3], None) == F.WS_ERR_BAD_ARG
    assert host(h, a[0], 8, 8, 8, a[1], 1, o, a[4], U8, 8, a[2], None, None) == F.WS_ERR_BAD_ARG
    assert host(h, a[0], 8, 8, 8, a[1], 1, o, a[4], U8, 7, a[2], a[3], None) == F.WS_ERR_BAD_ARG
    assert host(h, a[0], 8, 8, 8, a[1], 1, o, a[4], F.WS_DTYPES["float64"], 8, a[2], a[3], None) == F.WS_ERR_UNSUPPORTED
    bad = eng.options(max_level=255)
    assert dev(h, i, 32, 32, 32, s, ns, ctypes.byref(bad), w, U16, 32, t, r, None) == F.WS_ERR_MAX_TOO_HIGH
    bad = eng.options(max_level=0)
    assert host(h, a[0], 8, 8, 8, a[1], 1, ctypes.byref(bad), a[4], U8, 8, a[2], a[3], None) == F.WS_ERR_MAX_TOO_LOW
    torch.cuda.synchronize()
    assert bool((tree == 7).all()) and bool((raw == 7).all()) and (htree == 9).all() and (hrec == 9).all()
    # a transform in flight is refused
    out = torch.empty((32, 32), dtype=torch.int32, device=eng.device)
    eng.segment_begin(img, seeds, out)
    try:
        assert dev(h, i, 32, 32, 32, s, ns, o, w, U16, 32, t, r, None) == F.WS_ERR_BAD_ARG
        assert host(h, a[0], 8, 8, 8, a[1], 1, o, a[4], U8, 8, a[2], a[3], None) == F.WS_ERR_BAD_ARG
    finally:
        eng.segment_end()
    torch.cuda.synchronize()
    assert bool((tree == 7).all()) and bool((raw == 7).all()) and (htree == 9).all() and (hrec == 9).all()
    # the Python wrappers refuse what the library would
    with pytest.raises(TypeError):
        _ws(pkg).merge_tree_stats(himg, hseeds, weights=np.zeros((8, 8), dtype=np.float32))
    with pytest.raises(ValueError):
        _ws(pkg).merge_tree_stats(himg, hseeds, weights=np.zeros((8, 9), dtype=np.uint8))


def test_table_overflow_falls_back_to_memory(pkg, eng):
    """The own-statistics kernel keeps LAKE_SLOTS = 512 roots in a workgroup's LDS table (4 probes each) and a workgroup takes runs
    of 1024 consecutive pixels (one run here: a plane of up to 2048 x 1024 pixels gives every workgroup a single step).  The
    image is 255 everywhere, so nothing floods and every seed stays its own root for ever; the seeds are the checkerboard
    (r + c) even of a 32 x 64 plane.  Each of the two workgroups meets 16 rows x 32 seeds = 512 seed roots plus root 0 (the 512
    uncoloured pixels between them) = 513 distinct roots: one more than the 512 slots can hold however the probes fall, so at
    least one root of each workgroup -- with 4 probes, many -- finds no slot and updates memory itself.  Every seed's record
    must be its own pixel's, and record 0 the other pixels'."""
    h, w = 32, 64
    img = np.full((h, w), 255, dtype=np.uint8)
    rr, cc = np.nonzero((np.add.outer(np.arange(h), np.arange(w)) & 1) == 0)
    seeds = np.stack([rr, cc], axis=1)
    assert len(seeds) == 1024
    wt = np.random.default_rng(3).integers(0, 65536, (h, w), dtype=np.uint16)
    v = wt.astype(np.int64)
    want = ls.empty_records(len(seeds) + 1)
    for k, (r, c) in enumerate(seeds):
        want[k + 1] = ls.pixel_record(v, int(r), int(c))
    plane = np.zeros((h, w), dtype=np.int64)
    plane[rr, cc] = 1
    want[0] = ls.records_by_label(plane, v, 2)[0]
    tree, rec = _device_stats(eng, img, seeds, wt)
    assert (tree[1:, 1] == mt.ALIVE).all() and (tree[1:, 2] == 1).all() and tree[0, 2] == 1024
    assert ls.mismatch(rec, want) is None, ls.mismatch(rec, want)
    host = _ws(pkg).merge_tree_stats(img, seeds, weights=wt)[1]
    assert ls.mismatch(host, want) is None


@pytest.fixture(scope="module")
def big(eng):
    """2048^2 random field with u16 weights: tree, records, segmenting labels, stamps, weights (a workgroup takes two steps)."""
    import torch
    img = eng.random_field(2048, 2048, 11)
    seeds = eng.find_local_minima(img)
    wt = np.random.default_rng(11).integers(0, 65536, (2048, 2048), dtype=np.uint16)
    tree, raw, labels = eng.merge_tree_stats(img, seeds, weights=_weights_to_dev(eng, wt), want_labels=True)
    torch.cuda.synchronize()
    arr = eng.last_arrival().cpu().numpy().view(np.uint32)
    return (img, seeds, tree.cpu().numpy().view(np.uint32), ls.from_raw(raw.cpu().numpy()), labels.cpu().numpy().view(np.uint32), arr,
            wt.astype(np.int64))


LEVELS_AT_SIZE = [0, 61, 122, 200, 254]


def test_at_size_tree_is_merge_trees(eng, big):
    import torch
    img, seeds, tree, rec, labels, arr, v = big
    plain = eng.merge_tree(img, seeds)
    torch.cuda.synchronize()
    assert (plain.cpu().numpy().view(np.uint32) == tree).all()
    assert (rec["reserved"] == 0).all()


def test_at_size_survivors_and_record_zero_join_to_the_plane(big):
    img, seeds, tree, rec, labels, arr, v = big
    alive = (tree[:, 1] == mt.ALIVE) & (tree[:, 3] > 0)
    alive[0] = True
    got = ls.join(rec[alive])
    rows = np.arange(2048, dtype=np.int64)
    per_row, per_col = v.sum(axis=1), v.sum(axis=0)
    assert int(got["sum_w"]) == int(v.sum())
    assert int(got["sum_wr"]) == int((per_row * rows).sum()) and int(got["sum_wc"]) == int((per_col * rows).sum())
    assert int(got["sum_r"]) == int(got["sum_c"]) == 2048 * (2047 * 2048 // 2)
    assert (int(got["r_min"]), int(got["r_max"]), int(got["c_min"]), int(got["c_max"])) == (0, 2047, 0, 2047)
    assert int(got["w_min"]) == int(v.min()) and int(got["w_max"]) == int(v.max())
    assert int(got["peak_pixel"]) == int(np.argmax(v))          # (argmax: the first in row-major order)
    gone = tree[:, 3] == 0
    gone[0] = False
    assert (rec[gone] == ls.empty_records(1)[0]).all()


def test_at_size_every_record_is_own_part_plus_children(big):
    """Every record from its definition as a fold: own[c], the record of the pixels that arrive while c is the root of their
    colour, is recomputed here from the arrival stamps and the segmenting labels (the parent walk advanced level by level, as
    test_at_size_every_area_is_own_count_plus_children does for area); then record c == own[c] joined with the records of its
    children.  A colour that dies at level 0 hands on nothing and holds its seed pixel alone; record 0 is the uncoloured pixels'."""
    img, seeds, tree, rec, labels, arr, v = big
    parent, death = tree[:, 0].astype(np.int64), tree[:, 1].astype(np.int64)
    n_col = tree.shape[0]
    lab = labels.ravel().astype(np.int64)
    lvl = (arr.ravel() >> 24).astype(np.int64)
    coloured = (lab != 0) & (lvl != 0xFF)
    order = np.argsort(np.where(coloured, lvl, 256), kind="stable")
    first = np.searchsorted(np.where(coloured, lvl, 256)[order], np.arange(257))
    root = np.arange(n_col, dtype=np.int64)
    at_arrival = np.zeros(lab.size, dtype=np.int64)          # uncoloured pixels: record 0
    for t in range(255):
        dead = np.flatnonzero(death[root] <= t)
        while dead.size:
            root[dead] = parent[root[dead]]
            dead = dead[death[root[dead]] <= t]
        px = order[first[t]:first[t + 1]]
        at_arrival[px] = root[lab[px]]
    own = ls.records_by_key(at_arrival, v.ravel(), np.arange(lab.size), 2048, n_col)
    at0 = death == 0
    hands = np.flatnonzero((death != mt.ALIVE) & ~at0)
    kids = ls.join_by_key(parent[hands], rec[hands], n_col)
    want = ls.join_pairwise(own, kids)
    sy, sx = seeds.cpu().numpy()[:, 0].astype(np.int64), seeds.cpu().numpy()[:, 1].astype(np.int64)
    for c in np.flatnonzero(at0):
        assert tree[c, 3] == 1
        want[c] = ls.pixel_record(v, int(sy[c - 1]), int(sx[c - 1]))
    assert at0.sum() > 0 and hands.size > 100000
    assert ls.mismatch(rec, want) is None, ls.mismatch(rec, want)
    assert (own[at0]["sum_r"] == 0).all()


def test_at_size_dying_colours_hold_their_region_of_the_history_plane(eng, big):
    import torch
    img, seeds, tree, rec, labels, arr, v = big
    planes = eng.transform_history(img, seeds, levels=LEVELS_AT_SIZE, merging=True)
    torch.cuda.synchronize()
    planes = planes.cpu().numpy().view(np.uint32)
    death = tree[:, 1]
    idx = np.arange(2048 * 2048)
    for k, L in enumerate(LEVELS_AT_SIZE):
        last = np.flatnonzero(death == L + 1) if L < 254 else np.flatnonzero((death == mt.ALIVE) & (tree[:, 3] > 0))
        assert last.size
        mine = np.zeros(tree.shape[0], dtype=bool)
        mine[last] = True
        flat = planes[k].ravel()
        sel = mine[flat]
        want = ls.records_by_key(flat[sel], v.ravel()[sel], idx[sel], 2048, tree.shape[0])
        assert ls.mismatch(rec[last], want[last]) is None, (L, ls.mismatch(rec[last], want[last]))
    # record 0: what the last plane leaves uncoloured
    unc = planes[-1].ravel() == 0
    want0 = ls.records_by_key(np.zeros(int(unc.sum()), dtype=np.int64), v.ravel()[unc], idx[unc], 2048, 1)[0]
    assert rec[0] == want0


def _by_level_and_colour(lakes, offsets):
    rec = lakes.cpu().numpy()
    level = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets.astype(np.int64)))
    return rec[np.lexsort((rec[:, 0], level))]


def test_alternating_with_tree_history_and_list_on_one_context(eng):
    import torch
    img = eng.random_field(300, 420, 5)
    seeds = eng.find_local_minima(img)
    wt = _weights_to_dev(eng, np.random.default_rng(2).integers(0, 65536, (300, 420), dtype=np.uint16))
    levels = [3, 90, 254]
    tree0 = eng.merge_tree(img, seeds).clone()
    hist0 = eng.transform_history(img, seeds, levels=levels, merging=True).clone()
    lakes0, off0, unc0 = eng.transform_to_list(img, seeds, merging=True)
    lakes0 = _by_level_and_colour(lakes0, off0)
    stats0 = [x.clone() for x in eng.merge_tree_stats(img, seeds, weights=wt)]
    assert torch.equal(stats0[0], tree0)
    for _ in range(3):
        got = eng.merge_tree_stats(img, seeds, weights=wt)
        assert torch.equal(got[0], tree0) and torch.equal(got[1], stats0[1])
        assert torch.equal(eng.transform_history(img, seeds, levels=levels, merging=True), hist0)
        got = eng.merge_tree_stats(img, seeds, weights=wt)
        assert torch.equal(got[0], tree0) and torch.equal(got[1], stats0[1])
        lakes, off, unc = eng.transform_to_list(img, seeds, merging=True)
        assert (off == off0).all() and (unc == unc0).all() and (_by_level_and_colour(lakes, off) == lakes0).all()
        got = eng.merge_tree_stats(img, seeds, weights=wt)
        assert torch.equal(got[0], tree0) and torch.equal(got[1], stats0[1])
        assert torch.equal(eng.merge_tree(img, seeds), tree0)
    assert torch.equal(eng.transform_history(img, seeds, levels=levels, merging=True), hist0)


def test_repeated_call_replays_the_graph_bit_identically(eng):
    import torch
    img = eng.random_field(512, 512, 8)
    seeds = eng.find_local_minima(img)
    tree = torch.empty((seeds.shape[0] + 1, 4), dtype=torch.int32, device=eng.device)
    raw = torch.empty((seeds.shape[0] + 1, 9), dtype=torch.int64, device=eng.device)
    first = [x.clone() for x in eng.merge_tree_stats(img, seeds, out=tree, out_stats=raw)]
    for _ in range(4):
        got = eng.merge_tree_stats(img, seeds, out=tree, out_stats=raw)
        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])
    # (as merge_tree: the last call replayed the level loop, one captured graph per group of 16 levels)
    assert eng.stats()["graph_launches"] >= 16
