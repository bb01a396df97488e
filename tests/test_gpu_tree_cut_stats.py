"""tree_cut with catalogue thresholds (ws_tree_cut_stats_device, ws_merge_tree_stats_cut) against tests/tree_cut_stats_ref.py, -m gpu:
every plane, record, offset and hidden count bit for bit.  The device inputs are the engine's own: merge_tree_stats(want_labels=True)
and last_arrival() of the same flood."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import lake_stats_ref as ls
import tree_cut_ref as tc
import tree_cut_stats_ref as ts

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A


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


def _flood(eng, name):
    """(field, tree, stats, keys, labels): the engine's own tree, catalogue, stamps and segmenting labels of a shared case."""
    import torch
    if name not in _FLOODS:
        f = ts.field(name)
        t_img = torch.from_numpy(f.img).to(eng.device)
        t_seeds = torch.from_numpy(f.seeds.astype(np.int32)).to(eng.device)
        wt = None
        if f.weights is not None:
            w = np.ascontiguousarray(f.weights)
            wt = torch.from_numpy(w.view(np.int16) if w.dtype == np.uint16 else w).to(eng.device)
        tree, stats, labels = eng.merge_tree_stats(t_img, t_seeds, weights=wt, max_level=f.max_level, edge=f.edge, seed_shift=f.seed_shift,
                                                   want_labels=True)
        keys = eng.last_arrival()
        torch.cuda.synchronize()
        assert (tree.cpu().numpy().view(np.uint32) == f.tree).all(), name
        assert ls.mismatch(ls.from_raw(stats.cpu().numpy()), f.stats) is None, name
        assert (labels.cpu().numpy().view(np.uint32) == f.seg).all(), name
        _FLOODS[name] = (f, tree, stats, keys, labels)
    return _FLOODS[name]


def _pcuts(pkg, cuts):
    return [pkg.Cut(*c.key()) for c in cuts]


def _compare(f, want, planes, lakes=None, offsets=None, hidden=None, tag=None):
    for k in range(len(want)):
        if planes is not None:
            bad = np.argwhere(planes[k] != want[k])
            assert bad.size == 0, (tag, f.name, k, bad[:4], planes[k][tuple(bad[0])], want[k][tuple(bad[0])])
    if lakes is not None:
        rec, offs, hid = tc.expected_lists(want, f.n_seeds)
        assert (np.asarray(offsets) == offs).all(), (tag, f.name, offsets, offs)
        assert (np.asarray(hidden) == hid).all(), (tag, f.name, hidden, hid)
        assert lakes.shape == rec.shape and (lakes == rec).all(), (tag, f.name)
        for k in range(len(want)):      # every pixel is hidden or in exactly one record
            assert int(hid[k]) + int(lakes[int(offs[k]): int(offs[k + 1]), 1].sum()) == f.seg.size


def _run(pkg, eng, name, cuts, tag=None):
    import torch
    f, tree, stats, keys, labels = _flood(eng, name)
    planes, lakes, offsets, hidden = eng.tree_cut(tree, keys, labels, _pcuts(pkg, cuts), want_lakes=True, stats=stats)
    torch.cuda.synchronize()
    _compare(f, [f.cut(c) for c in cuts], planes.cpu().numpy().view(np.uint32), lakes.cpu().numpy().view(np.uint64), offsets, hidden, tag)
    return planes


def _raw(pkg, eng, tree, stats, ns, keys, labels, h, w, cuts, out=None, stride=None, lakes=None, cap=0, host=None):
    """The C call as it stands: pointers (ints or None), returns the status.  A cut is (min_area, min_leaves, show_level,
    merge_level, min_sum_w, min_w_max, min_depth[, index of a reserved byte to spoil])."""
    arr = (pkg._ffi.LakeCut * max(len(cuts), 1))()
    for k, c in enumerate(cuts):
        arr[k].min_area, arr[k].min_leaves, arr[k].show_level, arr[k].merge_level, arr[k].min_sum_w, arr[k].min_w_max, arr[k].min_depth = c[:7]
        if len(c) > 7:
            arr[k].reserved[c[7]] = 1
    n, offs, hid = host if host is not None else (None, None, None)
    return pkg._ffi.lib().ws_tree_cut_stats_device(eng.ctx.handle, tree, stats, ns, keys, labels, h, w, arr, len(cuts), out,
                                                   h * w if stride is None else stride, lakes, cap, ctypes.byref(n) if n is not None else None,
                                                   offs.ctypes.data if offs is not None else None, hid.ctypes.data if hid is not None else None)


def _host_arrays(k):
    return ctypes.c_size_t(77), np.full(k + 1, 77, dtype=np.uint64), np.full(max(k, 1), 77, dtype=np.uint64)


# ---- the shared cases: mixed, unsorted and repeated cuts in one call, planes and lists ------------------------------------------------

@pytest.mark.parametrize("name", ["random48x52", "random48x52_u16", "random40x37_edge", "random40x37_edge_shift", "walls", "plateau", "adjacent"])
def test_cases_in_one_call(pkg, eng, name):
    import torch
    f, cuts = ts.cuts_of(name)
    _flood(eng, name)
    before = eng.last_arrival()
    many = _run(pkg, eng, name, cuts)
    assert torch.equal(eng.last_arrival(), before)      # the context's stamps are nobody's scratch
    # the same cuts one per call: a call with ONE catalogue table reads the records themselves, one with more packs keys first
    _, tree, stats, keys, labels = _flood(eng, name)
    for k, c in enumerate(cuts):
        one = eng.tree_cut(tree, keys, labels, _pcuts(pkg, [c]), stats=stats)
        assert torch.equal(one[0], many[k]), c


@pytest.mark.parametrize("name", ["staircase_u16max", "two_lakes_u16max"])
def test_sums_around_two_to_the_32_are_compared_in_64_bits(pkg, eng, name):
    import torch
    f, cuts = ts.cuts_of(name)
    many = _run(pkg, eng, name, cuts)
    _, tree, stats, keys, labels = _flood(eng, name)
    for k, c in enumerate(cuts):      # both forms of the table kernel compare in 64 bits: one catalogue table a call, and several
        assert torch.equal(eng.tree_cut(tree, keys, labels, _pcuts(pkg, [c]), stats=stats)[0], many[k]), c
    planes = many.cpu().numpy().view(np.uint32)
    if name == "staircase_u16max":      # 2^32 + 5 drops all 254 dead nodes; the largest dead sum keeps exactly one
        alive = np.flatnonzero(f.death[1:] == ts.ALIVE) + 1
        assert set(np.unique(planes[0])) <= set(alive.tolist()) | {0}
        assert np.setdiff1d(np.unique(planes[1]), np.unique(planes[0])).size == 1
    else:      # 2^32 - 1 keeps the dead lake, whose sum lies above 2^32; its sum + 1 drops it
        assert (planes[0] == 2).sum() == int(f.area[2]) and not (planes[1] == 2).any() and (planes[2] == planes[0]).all()


# ---- without catalogue thresholds it is ws_tree_cut_device ---------------------------------------------------------------------------

def test_zero_catalogue_thresholds_equal_tree_cut_device(pkg, eng):
    import torch
    f, tree, stats, keys, labels = _flood(eng, "random48x52")
    h, w = f.shape
    cuts = tc.RANDOM_CUTS
    pc = [pkg.Cut(*c.key()) for c in cuts]
    want = eng.tree_cut(tree, keys, labels, pc, want_lakes=True)
    with_stats = eng.tree_cut(tree, keys, labels, pc, want_lakes=True, stats=stats)
    raw = [c.key() + (0, 0, 0) for c in cuts]
    out = torch.full((len(cuts), h, w), FILL, dtype=torch.int32, device=eng.device)
    lakes = torch.full((want[1].shape[0] + 1, 2), FILL, dtype=torch.int64, device=eng.device)
    host = _host_arrays(len(cuts))
    rc = _raw(pkg, eng, tree.data_ptr(), None, f.n_seeds, keys.data_ptr(), labels.data_ptr(), h, w, raw, out=out.data_ptr(), lakes=lakes.data_ptr(),
              cap=lakes.shape[0], host=host)      # d_stats == NULL
    torch.cuda.synchronize()
    assert rc == 0 and host[0].value == want[1].shape[0]
    for got in (with_stats, (out, lakes[: host[0].value], host[1], host[2])):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert (np.asarray(got[2]) == want[2]).all() and (np.asarray(got[3]) == want[3]).all()
    assert (lakes[host[0].value:] == FILL).all()
    _compare(f.f, [f.f.cut(c) for c in cuts], want[0].cpu().numpy().view(np.uint32))


# ---- how many cuts -------------------------------------------------------------------------------------------------------------------

def test_thirty_two_cuts_and_thirty_three(pkg, eng):
    import torch
    f, tree, stats, keys, labels = _flood(eng, "random48x52")
    cuts = [ts.Cut(min_area=(k * 7) % 5, min_leaves=k % 2, show_level=254 - 9 * (k % 5), merge_level=(k * 37) % 255,
                   min_sum_w=(0, 335, 336, 893)[k % 4], min_w_max=(0, 0, 239, 250)[(k // 4) % 4], min_depth=(0, 30, 55, 0, 87)[k % 5]) for k in range(32)]
    assert len({c.key()[:2] + c.key()[4:] for c in cuts}) > 16      # many tables
    _run(pkg, eng, "random48x52", cuts)
    h, w = f.shape
    out = torch.full((33, h, w), FILL, dtype=torch.int32, device=eng.device)
    rc = _raw(pkg, eng, tree.data_ptr(), stats.data_ptr(), f.n_seeds, keys.data_ptr(), labels.data_ptr(), h, w, [(0, 0, 254, 0, 5, 0, 0)] * 33,
              out=out.data_ptr())
    torch.cuda.synchronize()
    assert rc == pkg._ffi.WS_ERR_BAD_ARG and (out == FILL).all()
    with pytest.raises(ValueError):
        eng.tree_cut(tree, keys, labels, [pkg.Cut(min_depth=1)] * 33, stats=stats)


# ---- store forms and views ------------------------------------------------------------------------------------------------------------

def test_store_forms(pkg, eng):
    import torch
    for name in ("random48x52", "random40x37_edge"):      # w = 52, and the padded w = 39: no row is a multiple of four pixels
        f, tree, stats, keys, labels = _flood(eng, name)
        h, w = f.shape
        n, ns = h * w, f.n_seeds
        cuts = ts.cuts_of(name)[1][:4]
        raw = [c.key() for c in cuts]
        want = np.stack([f.cut(c) for c in cuts])
        for stride, shift in ((n, 1), (n + 3, 0)):      # a plane off 16-byte alignment; a stride that is no multiple of four
            buf = torch.full((len(cuts) * stride + 8,), FILL, dtype=torch.int32, device=eng.device)
            rc = _raw(pkg, eng, tree.data_ptr(), stats.data_ptr(), ns, keys.data_ptr(), labels.data_ptr(), h, w, raw, out=buf.data_ptr() + 4 * shift,
                      stride=stride)
            torch.cuda.synchronize()
            assert rc == 0, (name, stride, shift)
            got = buf.cpu().numpy().view(np.uint32)
            for k in range(len(cuts)):
                at = shift + k * stride
                assert (got[at: at + n].reshape(h, w) == want[k]).all(), (name, stride, shift, k)
                assert (got[at + n: at + stride] == FILL).all()
            assert (got[:shift] == FILL).all() and (got[shift + len(cuts) * stride:] == FILL).all()
    assert tc.field("random40x37_edge").shape[1] % 4 != 0


def test_catalogue_view_off_16_byte_alignment(pkg, eng):
    import torch
    f, tree, stats, keys, labels = _flood(eng, "random48x52")
    cuts = ts.cuts_of("random48x52")[1]
    rows = f.n_seeds + 1
    buf = torch.zeros(rows * 9 + 3, dtype=torch.int64, device=eng.device)
    buf[1: 1 + rows * 9] = stats.reshape(-1)      # the records are 8-byte aligned and no more
    view = buf[1: 1 + rows * 9].view(rows, 9)
    assert view.data_ptr() % 16 == 8
    tbuf = torch.zeros(rows * 4 + 4, dtype=torch.int32, device=eng.device)
    tbuf[1: 1 + rows * 4] = tree.reshape(-1)
    got = eng.tree_cut(tbuf[1: 1 + rows * 4].view(rows, 4), keys, labels, _pcuts(pkg, cuts), stats=view)
    torch.cuda.synchronize()
    _compare(f, [f.cut(c) for c in cuts], got.cpu().numpy().view(np.uint32))
    for c in cuts[:2] + cuts[7:8]:      # one catalogue table a call: the table kernel reads the view itself
        got = eng.tree_cut(tree, keys, labels, _pcuts(pkg, [c]), stats=view)
        _compare(f, [f.cut(c)], got.cpu().numpy().view(np.uint32), tag=c)


# ---- refusals: none of these reaches a walk ---------------------------------------------------------------------------------------------

def test_refusals_leave_everything_untouched(pkg, eng):
    import torch
    f, tree, stats, keys, labels = _flood(eng, "random48x52")
    h, w = f.shape
    ns, BAD = f.n_seeds, pkg._ffi.WS_ERR_BAD_ARG
    out = torch.full((2, h, w), FILL, dtype=torch.int32, device=eng.device)
    lakes = torch.full((2 * ns, 2), FILL, dtype=torch.int64, device=eng.device)
    good = [(4, 0, 254, 0, 0, 0, 0), (0, 0, 254, 0, 336, 0, 55)]

    def refused(what, **kw):
        host = _host_arrays(2)
        args = dict(tree=tree.data_ptr(), stats=stats.data_ptr(), ns=ns, keys=keys.data_ptr(), labels=labels.data_ptr(), h=h, w=w, cuts=good,
                    out=out.data_ptr(), lakes=lakes.data_ptr(), cap=2 * ns, host=host)
        args.update(kw)
        rc = _raw(pkg, eng, **args)
        torch.cuda.synchronize()
        assert rc == BAD, (what, rc)
        assert (out == FILL).all() and (lakes == FILL).all(), what
        assert host[0].value == 77 and (host[1] == 77).all() and (host[2] == 77).all(), what
        # the context is usable: a good call follows
        cut = ts.Cut(min_sum_w=336, min_depth=55)
        _compare(f, [f.cut(cut)], eng.tree_cut(tree, keys, labels, _pcuts(pkg, [cut]), stats=stats).cpu().numpy().view(np.uint32), tag=what)

    for k, name in enumerate(("min_sum_w", "min_w_max", "min_depth")):
        cut = [0, 0, 254, 0, 0, 0, 0]
        cut[4 + k] = 1
        refused(name + " with null d_stats", stats=None, cuts=[good[0], tuple(cut)])
    refused("min_sum_w above 32 bits with null d_stats", stats=None, cuts=[(0, 0, 254, 0, 1 << 32, 0, 0)])
    for byte in range(6):
        refused("reserved[%d]" % byte, cuts=[good[1], good[0] + (byte,)])
    refused("show_level 255", cuts=[(4, 0, 255, 0, 1, 0, 0)])
    spoilt = f.tree.copy()
    c = int(np.flatnonzero(f.death != ts.ALIVE)[5])
    spoilt[c, 0] = c      # parent == c: no merge tree
    t_spoilt = torch.from_numpy(spoilt.view(np.int32)).to(eng.device)
    refused("a bad tree", tree=t_spoilt.data_ptr())
    refused("null tree", tree=None)
    refused("no output", out=None, lakes=None)
    # a begun transform
    t_img = torch.from_numpy(f.img).to(eng.device)
    t_seeds = torch.from_numpy(f.seeds.astype(np.int32)).to(eng.device)
    seg = torch.empty((h, w), dtype=torch.int32, device=eng.device)
    eng.segment_begin(t_img, t_seeds, seg)
    try:
        rc = _raw(pkg, eng, tree.data_ptr(), stats.data_ptr(), ns, keys.data_ptr(), labels.data_ptr(), h, w, good, out=out.data_ptr())
    finally:
        eng.segment_end()
    torch.cuda.synchronize()
    assert rc == BAD and (out == FILL).all()
    with pytest.raises(ValueError):      # the shim refuses before any device work
        eng.tree_cut(tree, keys, labels, [pkg.Cut(min_w_max=3)])


# ---- a catalogue of another flood: table, then walk, on those numbers ---------------------------------------------------------------

def test_a_catalogue_from_another_field_is_table_then_walk(pkg, eng):
    import torch
    f, tree, stats, keys, labels = _flood(eng, "random40x37")
    cuts = ts.cuts_of("random40x37")[1]
    other = ts.foreign_catalogue()
    t_other = torch.from_numpy(np.array(other).view(np.int64).reshape(-1, 9)).to(eng.device)
    planes, lakes, offsets, hidden = eng.tree_cut(tree, keys, labels, _pcuts(pkg, cuts), want_lakes=True, stats=t_other)
    torch.cuda.synchronize()
    want = [f.cut_with(other, c) for c in cuts]
    assert any((a != f.cut(c)).any() for a, c in zip(want, cuts))
    _compare(f, want, planes.cpu().numpy().view(np.uint32), lakes.cpu().numpy().view(np.uint64), offsets, hidden)
    for k, c in enumerate(cuts):      # ... and one catalogue table a call
        assert torch.equal(eng.tree_cut(tree, keys, labels, _pcuts(pkg, [c]), stats=t_other)[0], planes[k]), c


# ---- the host form --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["random48x52_u16", "random40x37_edge_shift"])
def test_host_form(pkg, name):
    f, cuts = ts.cuts_of(name)
    b = pkg.TransformBuilder.new().set_max_water_lvl(f.max_level)
    if f.edge:
        b.enable_edge_correction()
    if f.seed_shift:
        b.shift_seeds_into_padded_plane()
    ws = b.build_merging()
    want = [f.cut(c) for c in cuts]
    planes, tree, stats, (lakes, offsets, hidden) = ws.merge_tree_cut(f.img, f.seeds, _pcuts(pkg, cuts), want_tree=True, want_lakes=True,
                                                                      weights=f.weights, want_stats=True)
    assert planes.dtype == np.uint64 and planes.shape == (len(cuts),) + f.shape
    assert (np.stack([tree.parent, tree.death_level, tree.area, tree.n_leaves], axis=1) == f.tree).all()
    assert ls.mismatch(stats, f.stats) is None
    _compare(f, want, planes, lakes, offsets, hidden, tag="host")
    only = ws.merge_tree_cut(f.img, f.seeds, _pcuts(pkg, cuts[:2]), weights=f.weights)      # tree and stats are nullable
    _compare(f, want[:2], only, tag="host planes only")
    if f.weights is None:      # a catalogue threshold alone takes the route too: the image weighs
        _compare(f, want[:3], ws.merge_tree_cut(f.img, f.seeds, _pcuts(pkg, cuts[:3])), tag="host, no weights")


def test_host_form_refuses_before_the_transform(pkg):
    f, cuts = ts.cuts_of("random48x52")
    ws = pkg.TransformBuilder.new().build_merging()
    ctx = ws._ctx()
    arr = (pkg._ffi.LakeCut * 1)()
    arr[0].show_level, arr[0].min_depth, arr[0].reserved[3] = 254, 5, 1
    planes = np.full((1,) + f.shape, FILL, dtype=np.uint64)
    seeds = np.ascontiguousarray(f.seeds.astype(np.uint64))
    img = np.ascontiguousarray(f.img)
    rc = pkg._ffi.lib().ws_merge_tree_stats_cut(ctx.handle, img.ctypes.data, f.shape[0], f.shape[1], f.shape[1], seeds.ctypes.data, f.n_seeds,
                                                ctypes.byref(ws._opt), None, 0, 0, arr, 1, None, None, planes.ctypes.data, None, 0, None, None, None)
    assert rc == pkg._ffi.WS_ERR_BAD_ARG and (planes == FILL).all()
