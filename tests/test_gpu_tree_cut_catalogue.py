"""The cut catalogue (ws_tree_cut_catalogue_device, ws_merge_tree_cut_catalogue) against tests/tree_cut_catalogue_ref.py, -m gpu:
every plane, list record, region record, offset, hidden count and hidden record bit for bit.  The device inputs are the engine's
own: merge_tree_stats(want_labels=True) and last_arrival() of the same flood; the weight plane of the device form has the PLANE's
shape (under edge correction the image inside a ring of zeros)."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import lake_stats_ref as ls
import tree_cut_catalogue_ref as cc
import tree_cut_ref as tc

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
FILL64 = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def eng(pkg):
    import torch
    with torch.cuda.stream(torch.cuda.Stream(0)):      # a stream of its own: the level loops are captured and replayed
        yield importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


_FLOODS = {}


def _dev(eng, a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(eng.device)


def _flood(eng, name):
    """(field, tree, stats, keys, labels, plane weights): the engine's own tree, catalogue, stamps and segmenting labels of a shared
    case, and the weights over its plane as the device form takes them."""
    import torch
    if name not in _FLOODS:
        f = cc.field(name)
        wt = _dev(eng, f.weights) if f.weights is not None else None
        tree, stats, labels = eng.merge_tree_stats(_dev(eng, f.img), _dev(eng, f.seeds.astype(np.int32)), weights=wt, max_level=f.max_level,
                                                   edge=f.edge, seed_shift=f.seed_shift, want_labels=True)
        keys = eng.last_arrival()
        torch.cuda.synchronize()
        assert (tree.cpu().numpy().view(np.uint32) == f.tree).all(), name
        assert ls.mismatch(ls.from_raw(stats.cpu().numpy()), f.stats) is None, name
        assert (labels.cpu().numpy().view(np.uint32) == f.seg).all(), name
        _FLOODS[name] = (f, tree, stats, keys, labels, _dev(eng, cc.plane_weights_array(f)))
    return _FLOODS[name]


def _pcuts(pkg, cuts):
    return [pkg.Cut(*c.key()) for c in cuts]


def _same(tag, got, want):
    bad = ls.mismatch(np.asarray(got), np.asarray(want))
    assert bad is None, (tag,) + bad


def _check(tag, f, cuts, planes, lakes, region, offsets, hidden, hidden_stats):
    """One call's outputs (numpy; planes and hidden_stats may be None) against the reference."""
    w_lakes, w_region, w_offsets, w_hidden, w_hid = cc.expected(f, cuts)
    if planes is not None:
        for k, c in enumerate(cuts):
            assert (planes[k] == f.cut(c)).all(), (tag, f.name, c)
    assert (np.asarray(offsets) == w_offsets).all() and (np.asarray(hidden) == w_hidden).all(), (tag, f.name)
    assert lakes.shape == w_lakes.shape and (lakes == w_lakes).all(), (tag, f.name)
    _same((tag, f.name, "regions"), region, w_region)
    assert (region["reserved"] == 0).all()
    if hidden_stats is not None:
        _same((tag, f.name, "hidden"), hidden_stats, w_hid)


def _call(pkg, eng, name, cuts, **kw):
    """DeviceEngine.tree_cut_catalogue on a shared case, checked; returns its raw outputs."""
    import torch
    f, tree, stats, keys, labels, wt = _flood(eng, name)
    got = eng.tree_cut_catalogue(tree, keys, labels, _pcuts(pkg, cuts), wt, stats=stats, **kw)
    torch.cuda.synchronize()
    planes, lakes, region, offsets, hidden, hidden_stats = got
    _check(name, f, cuts, planes.cpu().numpy().view(np.uint32) if planes is not None else None, lakes.cpu().numpy().view(np.uint64),
           ls.from_raw(region.cpu().numpy()), offsets, hidden, ls.from_raw(hidden_stats))
    return got


def _lake_cuts(pkg, cuts):
    arr = (pkg._ffi.LakeCut * max(len(cuts), 1))()
    for k, c in enumerate(cuts):
        arr[k].min_area, arr[k].min_leaves, arr[k].show_level, arr[k].merge_level, arr[k].min_sum_w, arr[k].min_w_max, arr[k].min_depth = c.key()
    return arr


def _host_arrays(k):
    return ctypes.c_size_t(77), np.full(k + 1, 77, dtype=np.uint64), np.full(max(k, 1), 77, dtype=np.uint64)


def _raw(pkg, eng, tree, stats, ns, keys, labels, h, w, weight, dtype, wstride, cuts, out=None, stride=None, lakes=None, region=None, cap=0, host=None,
         hidden_stats=None):
    """The C call as it stands: pointers (ints or None), returns the status."""
    n, offs, hid = host if host is not None else (None, None, None)
    return pkg._ffi.lib().ws_tree_cut_catalogue_device(
        eng.ctx.handle, tree, stats, ns, keys, labels, h, w, weight, dtype, wstride, _lake_cuts(pkg, cuts), len(cuts), out,
        h * w if stride is None else stride, lakes, region, cap, ctypes.byref(n) if n is not None else None,
        offs.ctypes.data if offs is not None else None, hid.ctypes.data if hid is not None else None,
        hidden_stats.ctypes.data if hidden_stats is not None else None)


def _dtype_of(pkg, wt):
    import torch
    return pkg._ffi.WS_DTYPES["uint8" if wt.dtype == torch.uint8 else "uint16"]


# ---- the shared cases -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.ALL)
def test_cases_in_one_call(pkg, eng, name):
    import torch
    f, cuts = cc.cuts_of(name)
    _, tree, stats, keys, labels, wt = _flood(eng, name)
    before = eng.last_arrival()
    planes, lakes, region, offsets, hidden, hidden_stats = _call(pkg, eng, name, cuts)
    assert torch.equal(eng.last_arrival(), before)      # the context's stamps are nobody's scratch
    # planes, lists, offsets and hidden are ws_tree_cut_stats_device's on the same inputs
    old = eng.tree_cut(tree, keys, labels, _pcuts(pkg, cuts), want_lakes=True, stats=stats)
    torch.cuda.synchronize()
    assert torch.equal(planes, old[0]) and torch.equal(lakes, old[1])
    assert (np.asarray(offsets) == old[2]).all() and (np.asarray(hidden) == old[3]).all()
    # the areas of the lists are the pixel counts of the regions, and a repeated cut has identical records
    seen = {}
    for k, c in enumerate(cuts):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        if c.key() in seen:
            a, b, first = seen[c.key()]
            assert torch.equal(region[lo:hi], region[a:b]) and (hidden_stats[k] == hidden_stats[first]).all()
        seen.setdefault(c.key(), (lo, hi, k))


def test_thirty_two_cuts_with_repeats(pkg, eng):
    import torch
    planes, lakes, region, offsets, hidden, hidden_stats = _call(pkg, eng, "random48x52", cc.THIRTY_TWO)
    for at, of in cc.REPEATS_32:
        a, b = (int(offsets[at]), int(offsets[at + 1])), (int(offsets[of]), int(offsets[of + 1]))
        assert torch.equal(region[a[0]: a[1]], region[b[0]: b[1]]) and torch.equal(lakes[a[0]: a[1]], lakes[b[0]: b[1]])
        assert (hidden_stats[at] == hidden_stats[of]).all() and torch.equal(planes[at], planes[of])
    f, tree, stats, keys, labels, wt = _flood(eng, "random48x52")
    with pytest.raises(ValueError):
        eng.tree_cut_catalogue(tree, keys, labels, [pkg.Cut()] * 33, wt)
    with pytest.raises(ValueError):      # a catalogue threshold without the catalogue: the shim refuses before any device work
        eng.tree_cut_catalogue(tree, keys, labels, [pkg.Cut(min_w_max=3)], wt)


# ---- call forms -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["random48x52_u16", "random40x37_edge", "checker48x52"])
def test_without_planes(pkg, eng, name):
    f, cuts = cc.cuts_of(name)
    got = _call(pkg, eng, name, cuts, want_planes=False)      # d_out == NULL: the measuring walks for itself
    assert got[0] is None


def test_null_outputs_one_at_a_time(pkg, eng):
    import torch
    name = "random40x37_edge_shift"
    f, cuts = cc.cuts_of(name)
    _, tree, stats, keys, labels, wt = _flood(eng, name)
    h, w = f.shape
    ns, k, dt = f.n_seeds, len(cuts), _dtype_of(pkg, wt)
    want = cc.expected(f, cuts)
    cap = len(want[0])      # exactly enough
    args = (tree.data_ptr(), stats.data_ptr(), ns, keys.data_ptr(), labels.data_ptr(), h, w, wt.data_ptr(), dt, w, cuts)
    # hidden_stats == NULL
    lakes = torch.zeros((cap, 2), dtype=torch.int64, device=eng.device)
    region = torch.zeros((cap, 9), dtype=torch.int64, device=eng.device)
    host = _host_arrays(k)
    assert _raw(pkg, eng, *args, lakes=lakes.data_ptr(), region=region.data_ptr(), cap=cap, host=host) == 0
    torch.cuda.synchronize()
    assert host[0].value == cap
    _check("no hidden_stats", f, cuts, None, lakes.cpu().numpy().view(np.uint64), ls.from_raw(region.cpu().numpy()), host[1], host[2], None)
    # d_region_stats == NULL, with and without lists: the hidden records alone
    for with_lists in (True, False):
        out = torch.full((k, h, w), FILL, dtype=torch.int32, device=eng.device)
        hs = ls.empty_records(k)
        host = _host_arrays(k)
        rc = _raw(pkg, eng, *args, out=out.data_ptr(), lakes=lakes.data_ptr() if with_lists else None, cap=cap, host=host if with_lists else None,
                  hidden_stats=hs)
        torch.cuda.synchronize()
        assert rc == 0
        _same(("hidden alone", with_lists), hs, want[4])
        assert (out.cpu().numpy().view(np.uint32) == np.stack([f.cut(c) for c in cuts])).all()
        if with_lists:
            assert (lakes.cpu().numpy().view(np.uint64) == want[0]).all() and (host[2] == want[3]).all()


def test_both_new_outputs_null_is_tree_cut_stats_device(pkg, eng):
    import torch
    name = "random48x52"
    f, cuts = cc.cuts_of(name)
    _, tree, stats, keys, labels, wt = _flood(eng, name)
    h, w = f.shape
    k = len(cuts)
    old = eng.tree_cut(tree, keys, labels, _pcuts(pkg, cuts), want_lakes=True, stats=stats)
    out = torch.full((k, h, w), FILL, dtype=torch.int32, device=eng.device)
    lakes = torch.full((old[1].shape[0] + 1, 2), FILL, dtype=torch.int64, device=eng.device)
    host = _host_arrays(k)
    # (the weight arguments are not looked at: a null plane of a dtype that does not exist)
    rc = _raw(pkg, eng, tree.data_ptr(), stats.data_ptr(), f.n_seeds, keys.data_ptr(), labels.data_ptr(), h, w, None, 99, 0, cuts, out=out.data_ptr(),
              lakes=lakes.data_ptr(), cap=lakes.shape[0], host=host)
    torch.cuda.synchronize()
    assert rc == 0 and host[0].value == old[1].shape[0]
    assert torch.equal(out, old[0]) and torch.equal(lakes[: host[0].value], old[1]) and (lakes[host[0].value:] == FILL).all()
    assert (host[1] == old[2]).all() and (host[2] == old[3]).all()


def test_views_off_alignment_and_odd_strides(pkg, eng):
    import torch
    for name in ("random48x52", "random40x37_edge"):      # w = 52, and the padded w = 39: no row is a multiple of four pixels
        f, cuts = cc.cuts_of(name)
        cuts = cuts[:5]
        _, tree, stats, keys, labels, wt = _flood(eng, name)
        h, w = f.shape
        n, ns, k, dt = h * w, f.n_seeds, len(cuts), _dtype_of(pkg, wt)
        want = cc.expected(f, cuts)
        cap = len(want[0]) + 2
        # keys and labels as views 4 bytes off 16-byte alignment; a weight plane with a row stride of w + 3
        kbuf = torch.zeros(n + 4, dtype=torch.int32, device=eng.device)
        lbuf = torch.zeros(n + 4, dtype=torch.int32, device=eng.device)
        kbuf[1: 1 + n], lbuf[1: 1 + n] = keys.reshape(-1), labels.reshape(-1)
        wbuf = torch.zeros((h, w + 3), dtype=wt.dtype, device=eng.device)
        wbuf[:, :w] = wt
        for stride, shift in ((n, 1), (n + 3, 0)):      # planes off 16-byte alignment; a stride that is no multiple of four
            buf = torch.full((k * stride + 8,), FILL, dtype=torch.int32, device=eng.device)
            lakes = torch.full((cap, 2), FILL, dtype=torch.int64, device=eng.device)
            rbuf = torch.full((cap * 9 + 3,), FILL64, dtype=torch.int64, device=eng.device)      # records 8-byte and not 16-byte aligned
            rptr = rbuf.data_ptr() + 8 if rbuf.data_ptr() % 16 == 0 else rbuf.data_ptr()
            r0 = (rptr - rbuf.data_ptr()) // 8
            assert rptr % 16 == 8
            host, hs = _host_arrays(k), ls.empty_records(k)
            rc = _raw(pkg, eng, tree.data_ptr(), stats.data_ptr(), ns, kbuf.data_ptr() + 4, lbuf.data_ptr() + 4, h, w, wbuf.data_ptr(), dt, w + 3, cuts,
                      out=buf.data_ptr() + 4 * shift, stride=stride, lakes=lakes.data_ptr(), region=rptr, cap=cap, host=host, hidden_stats=hs)
            torch.cuda.synchronize()
            assert rc == 0 and host[0].value == cap - 2, (name, stride, shift)
            got = buf.cpu().numpy().view(np.uint32)
            planes = np.stack([got[shift + j * stride: shift + j * stride + n].reshape(h, w) for j in range(k)])
            for j in range(k):
                assert (got[shift + j * stride + n: shift + (j + 1) * stride] == FILL).all()
            assert (got[:shift] == FILL).all() and (got[shift + k * stride:] == FILL).all()
            raw = rbuf.cpu().numpy()
            _check((name, stride, shift), f, cuts, planes, lakes[: cap - 2].cpu().numpy().view(np.uint64),
                   ls.from_raw(raw[r0: r0 + (cap - 2) * 9].reshape(-1, 9)), host[1], host[2], hs)
            assert (raw[:r0].view(np.uint64) == FILL64).all() and (raw[r0 + (cap - 2) * 9:].view(np.uint64) == FILL64).all()
            assert (lakes[cap - 2:] == FILL).all()
    assert tc.field("random40x37_edge").shape[1] % 4 != 0


# ---- capacity and refusals --------------------------------------------------------------------------------------------------------------

def test_capacity_one_short(pkg, eng):
    import torch
    name = "random48x52"
    f, cuts = cc.cuts_of(name)
    _, tree, stats, keys, labels, wt = _flood(eng, name)
    h, w = f.shape
    total = len(cc.expected(f, cuts)[0])
    lakes = torch.full((total, 2), FILL, dtype=torch.int64, device=eng.device)
    region = torch.full((total, 9), FILL64, dtype=torch.int64, device=eng.device)
    host, hs = _host_arrays(len(cuts)), ls.empty_records(len(cuts))
    rc = _raw(pkg, eng, tree.data_ptr(), stats.data_ptr(), f.n_seeds, keys.data_ptr(), labels.data_ptr(), h, w, wt.data_ptr(), _dtype_of(pkg, wt), w, cuts,
              lakes=lakes.data_ptr(), region=region.data_ptr(), cap=total - 1, host=host, hidden_stats=hs)
    torch.cuda.synchronize()
    assert rc == pkg._ffi.WS_ERR_CAPACITY and host[0].value == total
    assert (region.cpu().numpy().view(np.uint64) == FILL64).all()      # no measuring kernel has run
    _call(pkg, eng, name, cuts[:3])      # the context is usable


def test_refusals_leave_everything_untouched(pkg, eng):
    import torch
    name = "random48x52"
    f, cuts = cc.cuts_of(name)
    cuts = cuts[:2]
    _, tree, stats, keys, labels, wt = _flood(eng, name)
    h, w = f.shape
    ns, BAD, dt = f.n_seeds, pkg._ffi.WS_ERR_BAD_ARG, _dtype_of(pkg, wt)
    out = torch.full((2, h, w), FILL, dtype=torch.int32, device=eng.device)
    lakes = torch.full((2 * ns, 2), FILL, dtype=torch.int64, device=eng.device)
    region = torch.full((2 * ns, 9), FILL64, dtype=torch.int64, device=eng.device)

    def refused(what, code=BAD, **kw):
        host, hs = _host_arrays(2), np.full(2 * 9, FILL64, dtype=np.uint64)
        args = dict(tree=tree.data_ptr(), stats=stats.data_ptr(), ns=ns, keys=keys.data_ptr(), labels=labels.data_ptr(), h=h, w=w, weight=wt.data_ptr(),
                    dtype=dt, wstride=w, cuts=cuts, out=out.data_ptr(), lakes=lakes.data_ptr(), region=region.data_ptr(), cap=2 * ns, host=host,
                    hidden_stats=hs)
        args.update(kw)
        if args["lakes"] is None:
            args["host"] = None
        rc = _raw(pkg, eng, **args)
        torch.cuda.synchronize()
        assert rc == code, (what, rc)
        assert (out == FILL).all() and (lakes == FILL).all() and (region.cpu().numpy().view(np.uint64) == FILL64).all(), what
        assert host[0].value == 77 and (host[1] == 77).all() and (host[2] == 77).all() and (hs == FILL64).all(), what

    refused("d_region_stats without d_lakes", lakes=None)
    refused("null weight", weight=None)
    refused("short weight stride", wstride=w - 1)
    refused("bad dtype", code=pkg._ffi.WS_ERR_UNSUPPORTED, dtype=pkg._ffi.WS_DTYPES["float32"])
    refused("a catalogue threshold with null d_stats", stats=None, cuts=[cc.Cut(min_depth=3)])
    refused("null tree", tree=None)
    # a begun transform
    seg = torch.empty((h, w), dtype=torch.int32, device=eng.device)
    eng.segment_begin(_dev(eng, f.img), _dev(eng, f.seeds.astype(np.int32)), seg)
    try:
        refused("a begun transform")
    finally:
        eng.segment_end()
    _call(pkg, eng, name, cuts)      # the context is usable: a good call follows


# ---- empty and large cases --------------------------------------------------------------------------------------------------------------

def test_no_seeds_folds_the_whole_plane(pkg, eng):
    import torch
    h, w = 37, 41
    v = (np.arange(h * w, dtype=np.int64).reshape(h, w) * 7 % 251).astype(np.uint8)
    keys = torch.full((h, w), -(1 << 24), dtype=torch.int32, device=eng.device)      # 0xFF000000: never coloured
    labels = torch.zeros((h, w), dtype=torch.int32, device=eng.device)
    tree = torch.tensor([[0, -1, h * w, 0]], dtype=torch.int32, device=eng.device)
    planes, lakes, region, offsets, hidden, hidden_stats = eng.tree_cut_catalogue(tree, keys, labels, [pkg.Cut(), pkg.Cut(min_area=3), pkg.Cut(show_level=9)],
                                                                                  _dev(eng, v))
    torch.cuda.synchronize()
    assert lakes.shape[0] == 0 and region.shape[0] == 0 and (offsets == 0).all() and (hidden == h * w).all() and not planes.any()
    # closed form: the sums of the plane, its box, its extrema and the first pixel of the largest weight
    r, c = np.indices((h, w))
    whole = ls.empty_records(1)
    whole[0] = (v.sum(), (v * r).sum(), (v * c).sum(), r.sum(), c.sum(), 0, h - 1, 0, w - 1, v.min(), v.max(), int(np.flatnonzero(v.ravel() == v.max())[0]), 0)
    for k in range(3):
        _same(("no seeds", k), ls.from_raw(hidden_stats)[k: k + 1], whole)
    empty = eng.tree_cut_catalogue(tree, keys[:0], labels[:0], [pkg.Cut()], _dev(eng, v[:0]))      # no pixel: the identity
    _same("no pixel", ls.from_raw(empty[5]), ls.empty_records(1))


def test_a_workgroup_carries_its_table_across_steps(pkg, eng):
    """2056 x 2052: 4121 runs of 1024 pixels, past the 4096 workgroups of a call, so a workgroup takes two steps.  Expected: the
    numpy fold of the planes the same call returned (the render the existing tests hold right)."""
    import torch
    h, w = 2056, 2052
    assert (h * w + 1023) // 1024 > 4096
    img = eng.random_field(h, w, 5)
    seeds = eng.find_local_minima(img)
    tree, stats, labels = eng.merge_tree_stats(img, seeds, want_labels=True)
    keys = eng.last_arrival()
    ns = int(seeds.shape[0])
    cuts = [pkg.Cut(), pkg.Cut(min_area=12), pkg.Cut(show_level=120, merge_level=60), pkg.Cut(min_depth=20, merge_level=30)]
    planes, lakes, region, offsets, hidden, hidden_stats = eng.tree_cut_catalogue(tree, keys, labels, cuts, img, stats=stats)
    torch.cuda.synchronize()
    v = img.cpu().numpy()
    got, got_lakes, hs = ls.from_raw(region.cpu().numpy()), lakes.cpu().numpy().view(np.uint64), ls.from_raw(hidden_stats)
    for k in range(len(cuts)):
        plane = planes[k].cpu().numpy().view(np.uint32)
        rec = ls.records_by_label(plane, v, ns + 1)
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        cols, counts, hid = tc.lists_of(plane, ns)
        assert (got_lakes[lo:hi, 0] == cols).all() and (got_lakes[lo:hi, 1] == counts).all() and int(hidden[k]) == hid      # areas = pixel counts
        _same(("large", k), got[lo:hi], rec[cols.astype(np.int64)])
        _same(("large hidden", k), hs[k: k + 1], rec[:1])


# ---- the host form, the shim, centroids and the torch method ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["random40x37_edge_shift", "staircase_u16max"])
def test_host_form_and_shim(pkg, eng, name):
    import torch
    f, cuts = cc.cuts_of(name)
    b = pkg.TransformBuilder.new().set_max_water_lvl(f.max_level)
    if f.edge:
        b.enable_edge_correction()
    if f.seed_shift:
        b.shift_seeds_into_padded_plane()
    ws = b.build_merging()
    planes, lakes, region, offsets, hidden, hidden_stats, tree, stats = ws.merge_tree_cut_catalogue(f.img, f.seeds, _pcuts(pkg, cuts), weights=f.weights,
                                                                                                    want_tree=True, want_stats=True)
    assert planes.dtype == np.uint64 and planes.shape == (len(cuts),) + f.shape
    assert (np.stack([tree.parent, tree.death_level, tree.area, tree.n_leaves], axis=1) == f.tree).all()
    assert ls.mismatch(stats, f.stats) is None
    _check("host", f, cuts, planes, lakes, region, offsets, hidden, hidden_stats)
    # ... and the device form (the torch method) returns the same records
    dev = _call(pkg, eng, name, cuts)
    torch.cuda.synchronize()
    _same("host vs device", region, ls.from_raw(dev[2].cpu().numpy()))
    _same("host vs device, hidden", hidden_stats, ls.from_raw(dev[5]))
    # centroids takes the region records unchanged
    row, col = pkg.centroids(region)
    want = cc.expected(f, cuts)[1]
    sw = want["sum_w"].astype(np.float64)
    ok = sw > 0
    assert row.shape == (len(region),) and np.isnan(row[~ok]).all() and np.isnan(col[~ok]).all()
    assert (row[ok] == want["sum_wr"][ok].astype(np.float64) / sw[ok]).all() and (col[ok] == want["sum_wc"][ok].astype(np.float64) / sw[ok]).all()
    assert ((row[ok] >= want["r_min"][ok]) & (row[ok] <= want["r_max"][ok])).all()
    # without planes, tree and stats
    only = ws.merge_tree_cut_catalogue(f.img, f.seeds, _pcuts(pkg, cuts[:2]), weights=f.weights, want_planes=False)
    assert only[0] is None and len(only) == 6
    _check("host, lists only", f, cuts[:2], None, *only[1:])
    if f.weights is None:
        assert f.edge      # (the image weighs, inside a ring of zeros: the reference's plane_weights)


def test_host_form_refuses_before_the_transform(pkg):
    f, cuts = cc.cuts_of("random48x52")
    ws = pkg.TransformBuilder.new().build_merging()
    ctx = ws._ctx()
    arr = _lake_cuts(pkg, cuts[:1])
    planes = np.full((1,) + f.shape, FILL, dtype=np.uint64)
    region = np.full(9 * f.n_seeds, FILL64, dtype=np.uint64)
    seeds = np.ascontiguousarray(f.seeds.astype(np.uint64))
    img = np.ascontiguousarray(f.img)
    rc = pkg._ffi.lib().ws_merge_tree_cut_catalogue(ctx.handle, img.ctypes.data, f.shape[0], f.shape[1], f.shape[1], seeds.ctypes.data, f.n_seeds,
                                                    ctypes.byref(ws._opt), None, 0, 0, arr, 1, None, None, planes.ctypes.data, None, region.ctypes.data,
                                                    f.n_seeds, None, None, None, None)      # region_stats without lakes
    assert rc == pkg._ffi.WS_ERR_BAD_ARG and (planes == FILL).all() and (region == FILL64).all()
