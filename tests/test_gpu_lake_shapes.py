"""merge_tree_shapes (ws_merge_tree_shapes_device, ws_merge_tree_shapes, ws_merge_tree_shapes_from_arrival_device), -m gpu: all
twelve words of every record against the Python-integer reference of tests/lake_shapes_ref.py over the CPU oracle's planes, the
tree and the statistics byte for byte against ws_merge_tree_stats_device on the same context, the three forms against each
other.  tests/test_lake_shapes_cpu.py proves what the cases of tests/lake_shapes_cases.py are there for.  Every comparison is on
integers and exact, except the end-to-end check of api.ellipses."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import lake_shapes_cases as lc
import lake_shapes_ref as sh
import merge_tree_ref as mt
import oracle_lib as ol

pytestmark = pytest.mark.gpu
PAT = 0x5A5A5A5A5A5A5A5A


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


def _w_dev(eng, wt):
    """None, a u8 plane as it is, a u16 plane as its int16 bits."""
    import torch
    if wt is None:
        return None
    wt = np.ascontiguousarray(wt)
    return torch.from_numpy(wt if wt.dtype == np.uint8 else wt.view(np.int16)).to(eng.device)


def _np(t):
    return t.cpu().numpy()


def _same_bytes(a, b):
    return _np(a).tobytes() == _np(b).tobytes()


def _check(pkg, eng, r, tag, host=True, arrival=True):
    """Image form, arrival form and host form of the case r (lake_shapes_cases.Ref) against its reference and the stats call."""
    import torch
    t_img, t_seeds = _to_dev(eng, r.img, r.seeds)
    kw = dict(max_level=r.max_level, edge=r.edge, seed_shift=r.seed_shift)
    w = _w_dev(eng, r.weights)
    ref_tree, ref_stats = eng.merge_tree_stats(t_img, t_seeds, weights=w, **kw)
    tree, stats, shapes, labels = eng.merge_tree_shapes(t_img, t_seeds, weights=w, want_labels=True, **kw)
    torch.cuda.synchronize()
    assert (_np(tree).view(np.uint32) == r.tree).all(), (tag, "tree against the oracle")
    assert _same_bytes(tree, ref_tree) and _same_bytes(stats, ref_stats), (tag, "tree and stats against the stats call")
    assert sh.mismatch(_np(shapes), r.sums) is None, (tag, "device", sh.mismatch(_np(shapes), r.sums))
    if arrival:
        keys = eng.last_arrival()
        plane_w = r.weights if r.weights is not None else r.img      # this form has no image: its weights are the padded plane's
        plane_w = np.ascontiguousarray(np.pad(plane_w, 1)) if r.edge else plane_w
        a_tree, a_stats, a_shapes = eng.merge_tree_shapes_from_arrival(keys, labels, len(r.seeds), _w_dev(eng, plane_w), max_level=r.max_level)
        b_tree, b_stats = eng.merge_tree_from_arrival(keys, labels, len(r.seeds), max_level=r.max_level, weights=_w_dev(eng, plane_w), want_stats=True)
        torch.cuda.synchronize()
        assert _same_bytes(a_tree, b_tree) and _same_bytes(a_stats, b_stats) and _same_bytes(a_tree, tree) and _same_bytes(a_stats, stats), (tag, "arrival")
        assert _same_bytes(a_shapes, shapes), (tag, "arrival shapes")
    if host:
        got = _ws(pkg, r.max_level, r.edge, r.seed_shift).merge_tree_shapes(r.img, r.seeds, weights=r.weights)
        h_tree, h_stats, h_shapes = got
        assert h_shapes.dtype == pkg.api.LAKE_SHAPE_DTYPE and h_shapes.shape == (len(r.seeds) + 1,)
        assert (np.stack([h_tree.parent, h_tree.death_level, h_tree.area, h_tree.n_leaves], axis=1) == r.tree).all(), (tag, "host tree")
        assert h_stats.tobytes() == _np(stats).tobytes(), (tag, "host stats")
        assert sh.mismatch(h_shapes, r.sums) is None, (tag, "host", sh.mismatch(h_shapes, r.sums))
    return tree, stats, shapes, labels


@pytest.mark.parametrize("name", lc.FIELDS + ["duplicates", "walls"])
def test_random_fields_duplicates_and_walls(pkg, eng, name):
    _check(pkg, eng, lc.small(name), name)


@pytest.mark.parametrize("name", lc.CONSTRUCTED + ["three_seas"])
def test_constructed_cases(pkg, eng, name):
    _check(pkg, eng, lc.small(name), name, host=name in ("staircase", "three_seas"))


@pytest.mark.parametrize("maxlvl", [1, 60, 254])
def test_max_water_level(pkg, eng, maxlvl):
    img = cases.smooth_field(90, 110, 8)
    _check(pkg, eng, lc.Ref(img, ol.find_local_minima(img), lc.u16_plane(img.shape, 8), max_level=maxlvl), maxlvl)


def test_seed_shift(pkg, eng):
    img = cases.field(61, 83, 9)
    seeds = ol.find_local_minima(img)
    for shift in (True, False):
        _check(pkg, eng, lc.Ref(img, seeds, lc.u16_plane(img.shape, 9), edge=True, seed_shift=shift), shift)


def test_no_seeds_and_one_seed(pkg, eng):
    import torch
    img = cases.field(40, 52, 3)
    _check(pkg, eng, lc.Ref(img, [(20, 26)], lc.u16_plane(img.shape, 4)), "one seed")
    whole = sh.sums_of(np.zeros(img.shape, dtype=np.int64), sh.terms(img), [0])      # every pixel is uncoloured: record 0 is the plane's
    t_img = torch.from_numpy(img).to(eng.device)
    tree = torch.full((3, 4), 0x5A5A5A5A, dtype=torch.int32, device=eng.device)
    stats = torch.full((3, 9), PAT, dtype=torch.int64, device=eng.device)
    shapes = torch.full((3, 12), PAT, dtype=torch.int64, device=eng.device)
    opt = eng.options()
    rc = pkg._ffi.lib().ws_merge_tree_shapes_device(eng.ctx.handle, t_img.data_ptr(), 40, 52, 52, None, 0, ctypes.byref(opt), None, 0, 0,
                                                     tree.data_ptr(), stats.data_ptr(), shapes.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((tree[1:] == 0x5A5A5A5A).all()) and bool((stats[1:] == PAT).all()) and bool((shapes[1:] == PAT).all())
    assert _np(tree).view(np.uint32)[0].tolist() == [0, mt.ALIVE, 40 * 52, 0]
    assert sh.mismatch(_np(shapes[:1]), whole) is None and whole[0, 3] == 52 * sum(y * y for y in range(40))
    host = _ws(pkg).merge_tree_shapes(img, np.zeros((0, 2), dtype=np.uint64))
    assert host[2].shape == (1,) and sh.mismatch(host[2], whole) is None


@pytest.mark.parametrize("shape", lc.THIN)
def test_thin_planes_with_sums_past_64_bits(pkg, eng, shape):
    r = lc.thin(shape)
    tree, stats, shapes, labels = _check(pkg, eng, r, shape, host=False)
    assert (sh.from_words(_np(shapes)) >= 1 << 64).any()


def test_closed_form_plane_through_the_arrival_form(pkg, eng):
    """3 x (2^24 + 300), one colour, stamp 0 on its seed pixel and level 1 elsewhere, every weight 255: the sums in closed form,
    no oracle run.  A coordinate past 2^24 gives a term's product more than 64 bits' worth of partial products and the plain
    sums a high limb; the sum of v col^2 passes 2^64 sixty thousand times over.  With u16 weights of 65535 -- where one term
    would pass 2^64 -- the stats call's bound refuses the plane (test_lake_shapes_cpu), and so must this call, outputs untouched."""
    import torch
    h, w = lc.LINE
    keys, labels, w8, w16 = lc.line_planes()
    t_keys = torch.from_numpy(keys.view(np.int32)).to(eng.device)
    t_labels = torch.from_numpy(labels.view(np.int32)).to(eng.device)
    tree, stats, shapes = eng.merge_tree_shapes_from_arrival(t_keys, t_labels, 1, torch.from_numpy(w8).to(eng.device), max_level=1)
    b_tree, b_stats = eng.merge_tree_from_arrival(t_keys, t_labels, 1, max_level=1, weights=torch.from_numpy(w8).to(eng.device), want_stats=True)
    torch.cuda.synchronize()
    assert _same_bytes(tree, b_tree) and _same_bytes(stats, b_stats)
    assert _np(tree).view(np.uint32).tolist() == [[0, mt.ALIVE, 0, 0], [0, mt.ALIVE, h * w, 1]]
    want = np.array([[0] * 6, sh.closed_form_line_plane(h, w, 255)], dtype=object)
    assert sh.mismatch(_np(shapes), want) is None, sh.mismatch(_np(shapes), want)
    tree.fill_(7), stats.fill_(7), shapes.fill_(7)
    opt = eng.options(1, False)
    t16 = torch.from_numpy(w16.view(np.int16)).to(eng.device)
    rc = pkg._ffi.lib().ws_merge_tree_shapes_from_arrival_device(eng.ctx.handle, t_keys.data_ptr(), t_labels.data_ptr(), h, w, 1, ctypes.byref(opt),
                                                                  t16.data_ptr(), pkg._ffi.WS_DTYPES["uint16"], w, tree.data_ptr(), stats.data_ptr(),
                                                                  shapes.data_ptr())
    torch.cuda.synchronize()
    assert rc == pkg._ffi.WS_ERR_TOO_LARGE
    assert bool((tree == 7).all()) and bool((stats == 7).all()) and bool((shapes == 7).all())


def test_table_overflow_falls_back_to_memory(pkg, eng):
    """Each of the two workgroups meets 513 distinct roots in its one step, more than the table's slots
    (test_lake_shapes_cpu.test_overflow_case_has_more_roots_in_a_step_than_the_table_has_slots): the rest updates memory itself."""
    r = lc.small("overflow")
    _check(pkg, eng, r, "overflow")
    assert all(r.sums[k + 1].tolist() == sh.pixel_sums(sh.terms(r.v), 64, int(y), int(x)).tolist() for k, (y, x) in enumerate(r.seeds[:40]))


def test_unaligned_views(pkg, eng):
    """Stamp and label views off 16-byte alignment (the arrival form's scalar loads), a weight view with an odd row stride, and a
    d_shapes view at an 8-byte but not 16-byte offset."""
    import torch
    r = lc.small("field:50:70:2:0:u8")
    h, w = r.img.shape
    n = len(r.seeds)
    t_img, t_seeds = _to_dev(eng, r.img, r.seeds)
    tree, stats, shapes, labels = eng.merge_tree_shapes(t_img, t_seeds, weights=_w_dev(eng, r.weights), want_labels=True)
    keys = eng.last_arrival()
    kbuf = torch.zeros(h * w + 8, dtype=torch.int32, device=eng.device)
    lbuf = torch.zeros(h * w + 8, dtype=torch.int32, device=eng.device)
    kview, lview = kbuf[1:1 + h * w].view(h, w), lbuf[3:3 + h * w].view(h, w)
    kview.copy_(keys), lview.copy_(labels)
    assert kview.data_ptr() % 16 == 4 and lview.data_ptr() % 16 == 12
    wbuf = torch.zeros((h, w + 3), dtype=torch.uint8, device=eng.device)
    wview = wbuf[:, 1:1 + w]
    wview.copy_(torch.from_numpy(r.weights).to(eng.device))
    assert wview.stride(0) % 2 == 1
    sbuf = torch.full(((n + 1) * 12 + 4,), PAT, dtype=torch.int64, device=eng.device)
    base = 1 if sbuf.data_ptr() % 16 == 0 else 2
    sview = sbuf[base:base + (n + 1) * 12].view(n + 1, 12)
    assert sview.data_ptr() % 16 == 8
    a_tree, a_stats, a_shapes = eng.merge_tree_shapes_from_arrival(kview, lview, n, wview, out_shapes=sview)
    torch.cuda.synchronize()
    assert a_shapes.data_ptr() == sview.data_ptr()
    assert _same_bytes(a_tree, tree) and _same_bytes(a_stats, stats) and _same_bytes(sview, shapes)
    assert bool((sbuf[:base] == PAT).all()) and bool((sbuf[base + (n + 1) * 12:] == PAT).all())
    assert sh.mismatch(_np(sview), r.sums) is None
    # the image form with the strided weight view and the offset records
    sview.fill_(PAT)
    eng.merge_tree_shapes(t_img, t_seeds, weights=wview, out_shapes=sview)
    torch.cuda.synchronize()
    assert _same_bytes(sview, shapes)
    # a d_shapes off 8-byte alignment is refused
    opt = eng.options()
    rc = pkg._ffi.lib().ws_merge_tree_shapes_device(eng.ctx.handle, t_img.data_ptr(), h, w, w, t_seeds.data_ptr(), n, ctypes.byref(opt), None, 0, 0,
                                                     tree.data_ptr(), stats.data_ptr(), sview.data_ptr() + 4, None)
    assert rc == pkg._ffi.WS_ERR_BAD_ARG


def test_argument_checks_come_before_device_work(pkg, eng):
    """Every refusal of the stats call, with all three outputs untouched."""
    import torch
    L, F = pkg._ffi.lib(), pkg._ffi
    img = eng.random_field(32, 32, 1)
    seeds = eng.find_local_minima(img)
    ns = seeds.shape[0]
    tree = torch.full((ns + 1, 4), 7, dtype=torch.int32, device=eng.device)
    raw = torch.full((ns + 1, 9), 7, dtype=torch.int64, device=eng.device)
    shp = torch.full((ns + 1, 12), 7, dtype=torch.int64, device=eng.device)
    wt = torch.zeros((32, 32), dtype=torch.int16, device=eng.device)
    keys = torch.zeros((32, 32), dtype=torch.int32, device=eng.device)
    opt = eng.options()
    o = ctypes.byref(opt)
    h = eng.ctx.handle
    U16, U8 = F.WS_DTYPES["uint16"], F.WS_DTYPES["uint8"]
    dev, arr, host = L.ws_merge_tree_shapes_device, L.ws_merge_tree_shapes_from_arrival_device, L.ws_merge_tree_shapes
    i, s, t, r, q, w, k = img.data_ptr(), seeds.data_ptr(), tree.data_ptr(), raw.data_ptr(), shp.data_ptr(), wt.data_ptr(), keys.data_ptr()
    B = F.WS_ERR_BAD_ARG
    assert dev(h, None, 32, 32, 32, s, ns, o, w, U16, 32, t, r, q, None) == B
    assert dev(h, i, 32, 32, 32, None, ns, o, w, U16, 32, t, r, q, None) == B
    assert dev(h, i, 32, 32, 32, s, ns, o, w, U16, 32, None, r, q, None) == B
    assert dev(h, i, 32, 32, 32, s, ns, o, w, U16, 32, t, None, q, None) == B
    assert dev(h, i, 32, 32, 32, s, ns, o, w, U16, 32, t, r, None, None) == B
    assert dev(h, i, 32, 32, 32, s, ns, None, w, U16, 32, t, r, q, None) == B
    assert dev(h, i, 32, 32, 16, s, ns, o, w, U16, 32, t, r, q, None) == B          # a short image stride
    assert dev(h, i, 32, 32, 32, s, ns, o, w, U16, 31, t, r, q, None) == B          # a short weight stride
    for bad_dtype in (F.WS_DTYPES["float32"], F.WS_DTYPES["int16"], F.WS_DTYPES["int32"], 17, -1):
        assert dev(h, i, 32, 32, 32, s, ns, o, w, bad_dtype, 32, t, r, q, None) == F.WS_ERR_UNSUPPORTED
        assert arr(h, k, k, 32, 32, ns, o, w, bad_dtype, 32, t, r, q) == F.WS_ERR_UNSUPPORTED
    bad = eng.options(max_level=255)
    assert dev(h, i, 32, 32, 32, s, ns, ctypes.byref(bad), w, U16, 32, t, r, q, None) == F.WS_ERR_MAX_TOO_HIGH
    assert arr(h, k, k, 32, 32, ns, ctypes.byref(bad), w, U16, 32, t, r, q) == F.WS_ERR_MAX_TOO_HIGH
    assert arr(h, None, k, 32, 32, ns, o, w, U16, 32, t, r, q) == B
    assert arr(h, k, None, 32, 32, ns, o, w, U16, 32, t, r, q) == B
    assert arr(h, k, k, 32, 32, ns, o, None, U16, 32, t, r, q) == B                 # this form has no image
    assert arr(h, k, k, 32, 32, ns, o, w, U16, 31, t, r, q) == B
    assert arr(h, k, k, 32, 32, ns, o, w, U16, 32, None, r, q) == B
    assert arr(h, k, k, 32, 32, ns, o, w, U16, 32, t, None, q) == B
    assert arr(h, k, k, 32, 32, ns, o, w, U16, 32, t, r, None) == B
    sweep = eng.options(engine=pkg.ENGINE_SWEEP)
    assert arr(h, k, k, 32, 32, ns, ctypes.byref(sweep), w, U16, 32, t, r, q) == F.WS_ERR_UNSUPPORTED
    himg = np.zeros((8, 8), dtype=np.uint8)
    hseeds = np.array([[1, 1]], dtype=np.uint64)
    htree = np.full((2, 4), 9, dtype=np.uint32)
    hrec = np.full(2 * 9, 9, dtype=np.uint64)
    hshp = np.full(2 * 12, 9, dtype=np.uint64)
    hw = np.zeros((8, 8), dtype=np.uint8)
    a = (himg.ctypes.data, hseeds.ctypes.data, htree.ctypes.data, hrec.ctypes.data, hw.ctypes.data, hshp.ctypes.data)
    assert host(h, None, 8, 8, 8, a[1], 1, o, a[4], U8, 8, a[2], a[3], a[5], None) == B
    assert host(h, a[0], 8, 8, 8, None, 1, o, a[4], U8, 8, a[2], a[3], a[5], None) == B
    assert host(h, a[0], 8, 8, 8, a[1], 1, o, a[4], U8, 8, None, a[3], a[5], None) == B
    assert host(h, a[0], 8, 8, 8, a[1], 1, o, a[4], U8, 8, a[2], None, a[5], None) == B
    assert host(h, a[0], 8, 8, 8, a[1], 1, o, a[4], U8, 8, a[2], a[3], None, None) == B
    assert host(h, a[0], 8, 8, 8, a[1], 1, o, a[4], U8, 7, a[2], a[3], a[5], None) == B
    assert host(h, a[0], 8, 8, 8, a[1], 1, o, a[4], F.WS_DTYPES["float64"], 8, a[2], a[3], a[5], None) == F.WS_ERR_UNSUPPORTED
    low = eng.options(max_level=0)
    assert host(h, a[0], 8, 8, 8, a[1], 1, ctypes.byref(low), a[4], U8, 8, a[2], a[3], a[5], None) == F.WS_ERR_MAX_TOO_LOW
    torch.cuda.synchronize()

    def untouched():
        return (bool((tree == 7).all()) and bool((raw == 7).all()) and bool((shp == 7).all()) and (htree == 9).all() and (hrec == 9).all()
                and (hshp == 9).all())
    assert untouched()
    out = torch.empty((32, 32), dtype=torch.int32, device=eng.device)      # a transform in flight is refused
    eng.segment_begin(img, seeds, out)
    try:
        assert dev(h, i, 32, 32, 32, s, ns, o, w, U16, 32, t, r, q, None) == B
        assert arr(h, k, k, 32, 32, ns, o, w, U16, 32, t, r, q) == B
        assert host(h, a[0], 8, 8, 8, a[1], 1, o, a[4], U8, 8, a[2], a[3], a[5], None) == B
    finally:
        eng.segment_end()
    torch.cuda.synchronize()
    assert untouched()
    # no pixel: the arrival form writes the identity
    assert arr(h, None, None, 0, 7, 0, o, w, U8, 7, t, r, q) == 0
    torch.cuda.synchronize()
    assert bool((shp[0] == 0).all()) and bool((shp[1:] == 7).all()) and _np(tree).view(np.uint32)[0].tolist() == [0, mt.ALIVE, 0, 0]
    with pytest.raises(TypeError):
        _ws(pkg).merge_tree_shapes(himg, hseeds, weights=np.zeros((8, 8), dtype=np.float32))
    with pytest.raises(ValueError):
        _ws(pkg).merge_tree_shapes(himg, hseeds, weights=np.zeros((8, 9), dtype=np.uint8))


def test_alternating_calls_on_one_context(pkg, eng):
    """Between merge_tree_stats, merge_tree, transform_history and tree_cut the shapes call changes nothing of theirs, and a
    repeated call replays bit-identically."""
    import torch
    r = lc.small("field:96:96:3:1:u16")
    t_img, t_seeds = _to_dev(eng, r.img, r.seeds)
    w = _w_dev(eng, r.weights)
    kw = dict(edge=True)
    tree0, stats0, labels0 = eng.merge_tree_stats(t_img, t_seeds, weights=w, want_labels=True, **kw)
    tree0, stats0, labels0 = tree0.clone(), stats0.clone(), labels0.clone()
    keys0 = eng.last_arrival().clone()
    hist0 = eng.transform_history(t_img, t_seeds, levels=[0, 100, 254], merging=True, **kw).clone()
    cut = pkg.Cut(min_area=20, show_level=200, merge_level=200)
    cut0 = eng.tree_cut(tree0, keys0, labels0, cut).clone()
    first = None
    for step in range(3):
        tree, stats, shapes = eng.merge_tree_shapes(t_img, t_seeds, weights=w, **kw)
        torch.cuda.synchronize()
        assert _same_bytes(tree, tree0) and _same_bytes(stats, stats0)
        if first is None:
            first = shapes.clone()
            assert sh.mismatch(_np(first), r.sums) is None
        assert _same_bytes(shapes, first), step
        assert _same_bytes(eng.last_arrival(), keys0)
        if step == 0:
            assert _same_bytes(eng.merge_tree(t_img, t_seeds, **kw), tree0)
        elif step == 1:
            assert _same_bytes(eng.transform_history(t_img, t_seeds, levels=[0, 100, 254], merging=True, **kw), hist0)
            assert _same_bytes(eng.tree_cut(tree0, keys0, labels0, cut), cut0)
        later = eng.merge_tree_stats(t_img, t_seeds, weights=w, **kw)
        torch.cuda.synchronize()
        assert _same_bytes(later[0], tree0) and _same_bytes(later[1], stats0), step


def test_ellipses_end_to_end(pkg, eng):
    """The shim, DeviceEngine and ellipses on one field: a lake's mask from the history plane, its moments directly in float64
    from centred coordinates (no cancellation), relative 1e-9."""
    import torch
    img = cases.field(80, 100, 12)
    seeds = ol.find_local_minima(img)
    wt = lc.u16_plane(img.shape, 12)
    mt_tree, stats, shapes, labels = _ws(pkg).merge_tree_shapes(img, seeds, weights=wt, want_labels=True)
    t_img, t_seeds = _to_dev(eng, img, seeds)
    d_tree, d_stats, d_shapes = eng.merge_tree_shapes(t_img, t_seeds, weights=_w_dev(eng, wt))
    torch.cuda.synchronize()
    assert _np(d_shapes).tobytes() == shapes.tobytes() and _np(d_stats).tobytes() == stats.tobytes()
    got = {True: pkg.ellipses(stats, shapes), False: pkg.ellipses(stats, shapes, weighted=False, area=mt_tree.area)}
    big = [c for c in np.argsort(-mt_tree.area.astype(np.int64)) if c != 0 and mt_tree.death_level[c] != mt.ALIVE and mt_tree.death_level[c] > 0][:4]
    big.append(int(np.flatnonzero(mt_tree.death_level[1:] == mt.ALIVE)[0]) + 1)
    for c in big:
        L = 254 if mt_tree.death_level[c] == mt.ALIVE else int(mt_tree.death_level[c]) - 1
        plane = _np(eng.transform_history(t_img, t_seeds, levels=[L], merging=True))[0]
        rr, cc = np.nonzero(plane == c)
        assert len(rr) == mt_tree.area[c]
        for weighted in (True, False):
            v = wt[rr, cc].astype(np.float64) if weighted else np.ones(len(rr))
            S = v.sum()
            dr, dc = rr - (v * rr).sum() / S, cc - (v * cc).sum() / S
            a, b, cv = (v * dr * dr).sum() / S, (v * dc * dc).sum() / S, (v * dr * dc).sum() / S
            var_r, var_c, cov, major, minor, angle = (x[c] for x in got[weighted])
            scale = max(a, b)
            assert abs(var_r - a) <= 1e-9 * scale and abs(var_c - b) <= 1e-9 * scale and abs(cov - cv) <= 1e-9 * scale
            lo, hi = np.linalg.eigvalsh(np.array([[a, cv], [cv, b]]))
            assert abs(major ** 2 - hi) <= 1e-9 * hi and abs(minor ** 2 - lo) <= 1e-9 * hi
            assert abs(np.tan(2 * angle) * (a - b) - 2 * cv) <= 1e-8 * scale * max(1.0, abs(np.tan(2 * angle)))


def test_at_size_every_record_is_its_own_part_plus_its_childrens(eng):
    """1024^2, u16 weights: record c less the records of its children (colours whose parent is c, death level from 1 up) is the
    sum over c's own pixels -- those whose colour's root at their arrival level is c, found with the tree's parents on the host."""
    import torch
    n = 1024
    img = eng.random_field(n, n, 5)
    seeds = eng.find_local_minima(img)
    wt = lc.u16_plane((n, n), 77)
    tree, stats, shapes, labels = eng.merge_tree_shapes(img, seeds, weights=_w_dev(eng, wt), want_labels=True)
    ref_tree, ref_stats = eng.merge_tree_stats(img, seeds, weights=_w_dev(eng, wt))
    keys = _np(eng.last_arrival()).view(np.uint32)
    torch.cuda.synchronize()
    assert _same_bytes(tree, ref_tree) and _same_bytes(stats, ref_stats)
    tree, labels = _np(tree).view(np.uint32), _np(labels).view(np.uint32).ravel().astype(np.int64)
    parent, death = tree[:, 0].astype(np.int64), tree[:, 1].astype(np.int64)
    arr = (keys.ravel() >> 24).astype(np.int64)
    coloured = (labels != 0) & (arr != 255)
    root = np.where(coloured, labels, 0)
    for _ in range(300):      # up the tree while the colour had died by the pixel's arrival level
        move = coloured & (death[root] <= arr)
        if not move.any():
            break
        root[move] = parent[root[move]]
    else:
        raise AssertionError("a parent chain longer than 300")
    # own sums as twelve exact limb sums in uint64, as the kernels keep them (a limb stays below 2^64: see ws_shape_part.hpp)
    y, x = np.divmod(np.arange(n * n, dtype=np.uint64), np.uint64(n))
    v = wt.ravel().astype(np.uint64)
    terms = [v * y * y, v * x * x, v * y * x, y * y, x * x, y * x]          # every term below 2^36
    ns = len(tree)
    own = np.zeros((ns, 6), dtype=object)
    for j, t in enumerate(terms):
        lo = np.bincount(root, weights=(t & np.uint64(0xFFFFF)).astype(np.float64), minlength=ns)      # 2^20 * 2^20 pixels: exact in a double
        hi = np.bincount(root, weights=(t >> np.uint64(20)).astype(np.float64), minlength=ns)          # 2^16 * 2^20
        own[:, j] = [int(a) + (int(b) << 20) for a, b in zip(lo, hi)]
    got = sh.from_words(_np(shapes))
    kids = np.zeros((ns, 6), dtype=object)
    dying = np.flatnonzero((death != mt.ALIVE) & (death > 0) & (tree[:, 3] > 0))
    for c in dying:
        kids[parent[c]] = kids[parent[c]] + got[c]
    exists = tree[:, 3] > 0
    exists[0] = True
    level0 = death == 0
    check = exists & ~level0
    assert (got[check] == (own + kids)[check]).all()
    assert not own[level0 & exists].any() and not got[~exists].any()
