"""tree_cut (ws_tree_cut_device, ws_merge_tree_cut) against tests/tree_cut_ref.py, -m gpu: every plane, record, offset and hidden
count bit for bit.  The device inputs are the engine's own: merge_tree(want_labels=True) and last_arrival() of the same flood."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import tree_cut_ref as tc

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
    """(field, tree, keys, labels): the engine's own tree, stamps and segmenting labels of a shared case, as device tensors."""
    import torch
    if name not in _FLOODS:
        f = tc.field(name)
        t_img = torch.from_numpy(f.img).to(eng.device)
        t_seeds = torch.from_numpy(f.seeds.astype(np.int32)).to(eng.device)
        tree, labels = eng.merge_tree(t_img, t_seeds, max_level=f.max_level, edge=f.edge, seed_shift=f.seed_shift, want_labels=True)
        keys = eng.last_arrival()
        torch.cuda.synchronize()
        assert (tree.cpu().numpy().view(np.uint32) == f.tree).all(), name
        assert (labels.cpu().numpy().view(np.uint32) == f.seg).all(), name
        assert ((keys.cpu().numpy().view(np.uint32) >> 24) == (f.keys32() >> 24)).all(), name
        _FLOODS[name] = (f, tree, keys, labels)
    return _FLOODS[name]


def _pcuts(pkg, cuts):
    return [pkg.Cut(c.min_area, c.min_leaves, c.show_level, c.merge_level) for c in cuts]


def _compare(f, cuts, planes, lakes=None, offsets=None, hidden=None, tag=None):
    want = [f.cut(c) for c in cuts]
    for k, c in enumerate(cuts):
        if planes is not None:
            bad = np.argwhere(planes[k] != want[k])
            assert bad.size == 0, (tag, f.name, c, bad[:4], planes[k][tuple(bad[0])], want[k][tuple(bad[0])])
    if lakes is not None:
        rec, offs, hid = tc.expected_lists(want, f.n_seeds)
        assert (np.asarray(offsets) == offs).all(), (tag, f.name, offsets, offs)
        assert (np.asarray(hidden) == hid).all(), (tag, f.name, hidden, hid)
        assert lakes.shape == rec.shape and (lakes == rec).all(), (tag, f.name)
        for k in range(len(cuts)):      # every pixel is hidden or in exactly one record
            assert int(hid[k]) + int(lakes[int(offs[k]): int(offs[k + 1]), 1].sum()) == f.seg.size


def _run(pkg, eng, name, cuts, tag=None):
    import torch
    f, tree, keys, labels = _flood(eng, name)
    planes, lakes, offsets, hidden = eng.tree_cut(tree, keys, labels, _pcuts(pkg, cuts), want_lakes=True)
    torch.cuda.synchronize()
    _compare(f, cuts, planes.cpu().numpy().view(np.uint32), lakes.cpu().numpy().view(np.uint64), offsets, hidden, tag)
    return planes


def _raw(pkg, eng, tree, ns, keys, labels, h, w, cuts, out=None, stride=None, lakes=None, cap=0, host=None, n_cuts=None):
    """The C call as it stands: pointers (ints or None), returns the status.  host: (n_lakes c_size_t, offsets, hidden) or None."""
    arr = (pkg._ffi.TreeCut * max(len(cuts), 1))()
    for k, c in enumerate(cuts):
        arr[k].min_area, arr[k].min_leaves, arr[k].show_level, arr[k].merge_level = c[0], c[1], c[2], c[3]
        if len(c) > 4:
            arr[k].reserved[0], arr[k].reserved[1] = c[4], c[5]
    n, offs, hid = host if host is not None else (None, None, None)
    return pkg._ffi.lib().ws_tree_cut_device(eng.ctx.handle, tree, ns, keys, labels, h, w, arr, len(cuts) if n_cuts is None else n_cuts, out,
                                             h * w if stride is None else stride, lakes, cap, ctypes.byref(n) if n is not None else None,
                                             offs.ctypes.data if offs is not None else None, hid.ctypes.data if hid is not None else None)


def _host_arrays(k):
    return ctypes.c_size_t(77), np.full(k + 1, 77, dtype=np.uint64), np.full(max(k, 1), 77, dtype=np.uint64)


# ---- the random field: many cuts in one call, one per call, the history planes ------------------------------------------------------

def test_random_field_many_cuts_in_one_call(pkg, eng):
    import torch
    f, tree, keys, labels = _flood(eng, "random48x52")
    before = eng.last_arrival()
    many = _run(pkg, eng, "random48x52", tc.RANDOM_CUTS)
    for k, c in enumerate(tc.RANDOM_CUTS):      # the same cuts one per call
        one = eng.tree_cut(tree, keys, labels, _pcuts(pkg, [c]))
        assert torch.equal(one[0], many[k]), c
    assert torch.equal(eng.last_arrival(), before)      # the context's stamps are nobody's scratch


def test_level_cuts_are_the_engine_s_history_planes(pkg, eng):
    import torch
    f, tree, keys, labels = _flood(eng, "random48x52")
    levels = [0, 50, 254]
    got = eng.tree_cut(tree, keys, labels, [pkg.Cut(show_level=L, merge_level=L) for L in levels])
    t_img = torch.from_numpy(f.img).to(eng.device)
    t_seeds = torch.from_numpy(f.seeds.astype(np.int32)).to(eng.device)
    hist = eng.transform_history(t_img, t_seeds, levels=levels, merging=True)
    assert torch.equal(got, hist)
    for k, L in enumerate(levels):
        assert (got[k].cpu().numpy().view(np.uint32) == f.planes[L]).all(), L


@pytest.mark.parametrize("name", ["random40x37", "random40x37_edge", "random40x37_edge_shift", "random33x64", "adjacent"])
def test_odd_widths_many_roots_and_padded_planes(pkg, eng, name):
    _run(pkg, eng, name, tc.MIXED_CUTS)


@pytest.mark.parametrize("name", ["plateau", "walls", "constant"])
def test_plateaus_walls_and_seed_lists_with_repeats(pkg, eng, name):
    _run(pkg, eng, name, tc.MIXED_CUTS)


def test_staircase_254_deep(pkg, eng):
    f = tc.field("staircase")
    _run(pkg, eng, "staircase", tc.staircase_cuts(f))


# ---- store and load forms -----------------------------------------------------------------------------------------------------------

def test_store_forms(pkg, eng):
    import torch
    f, tree, keys, labels = _flood(eng, "random48x52")
    h, w = f.shape
    n, ns = h * w, f.n_seeds
    cuts = tc.RANDOM_CUTS[:4]
    raw = [c.key() for c in cuts]
    want = np.stack([f.cut(c) for c in cuts])
    for stride, shift in ((n, 0), (n + 4, 0), (n, 1), (n + 3, 0)):      # 16-byte stores; the same with a gap; off alignment; an odd stride
        buf = torch.full((len(cuts) * stride + 8,), FILL, dtype=torch.int32, device=eng.device)
        rc = _raw(pkg, eng, tree.data_ptr(), ns, keys.data_ptr(), labels.data_ptr(), h, w, raw, out=buf.data_ptr() + 4 * shift, stride=stride)
        torch.cuda.synchronize()
        assert rc == 0, (stride, shift)
        got = buf.cpu().numpy().view(np.uint32)
        for k in range(len(cuts)):
            at = shift + k * stride
            assert (got[at: at + n].reshape(h, w) == want[k]).all(), (stride, shift, k)
            assert (got[at + n: at + stride] == FILL).all()      # the gap between planes is nobody's
        assert (got[:shift] == FILL).all() and (got[shift + len(cuts) * stride:] == FILL).all()
    # key and label views one word into larger buffers: scalar loads, the same planes
    kbuf = torch.zeros(n + 4, dtype=torch.int32, device=eng.device)
    lbuf = torch.zeros(n + 4, dtype=torch.int32, device=eng.device)
    kbuf[1: n + 1] = keys.reshape(-1)
    lbuf[1: n + 1] = labels.reshape(-1)
    got = eng.tree_cut(tree, kbuf[1: n + 1].view(h, w), lbuf[1: n + 1].view(h, w), _pcuts(pkg, cuts))
    assert (got.cpu().numpy().view(np.uint32) == want).all()
    # the records off 16-byte alignment too
    tbuf = torch.zeros((ns + 1) * 4 + 4, dtype=torch.int32, device=eng.device)
    tbuf[1: 1 + (ns + 1) * 4] = tree.reshape(-1)
    got = eng.tree_cut(tbuf[1: 1 + (ns + 1) * 4].view(ns + 1, 4), keys, labels, _pcuts(pkg, cuts))
    assert (got.cpu().numpy().view(np.uint32) == want).all()


@pytest.mark.parametrize("name", ["random1x3", "random3x1", "random257x4"])
def test_fewer_than_four_pixels_and_one_tail_block(pkg, eng, name):
    _run(pkg, eng, name, [tc.Cut(), tc.Cut(min_area=3), tc.Cut(show_level=1, merge_level=200)])


# ---- how many cuts, sizes, lists ----------------------------------------------------------------------------------------------------

def test_thirty_two_cuts_and_thirty_three(pkg, eng):
    import torch
    f, tree, keys, labels = _flood(eng, "random48x52")
    cuts = [tc.Cut(min_area=(k * 7) % 40, min_leaves=k % 3, show_level=254 - 9 * (k % 5), merge_level=(k * 37) % 255) for k in range(32)]
    _run(pkg, eng, "random48x52", cuts)
    h, w = f.shape
    out = torch.full((33, h, w), FILL, dtype=torch.int32, device=eng.device)
    rc = _raw(pkg, eng, tree.data_ptr(), f.n_seeds, keys.data_ptr(), labels.data_ptr(), h, w, [(0, 0, 254, 0)] * 33, out=out.data_ptr())
    torch.cuda.synchronize()
    assert rc == pkg._ffi.WS_ERR_BAD_ARG and (out == FILL).all()
    with pytest.raises(ValueError):
        eng.tree_cut(tree, keys, labels, [pkg.Cut()] * 33)


def test_no_seed_no_pixel_no_cut(pkg, eng):
    import torch
    f, tree, keys, labels = _flood(eng, "random48x52")
    h, w = f.shape
    # no seed: the tree is record 0 alone, nothing is shown
    none = torch.tensor([[0, -1, h * w, 0]], dtype=torch.int32, device=eng.device)
    zero = torch.zeros((h, w), dtype=torch.int32, device=eng.device)
    out = torch.full((2, h, w), FILL, dtype=torch.int32, device=eng.device)
    lakes = torch.full((4, 2), FILL, dtype=torch.int64, device=eng.device)
    host = _host_arrays(2)
    rc = _raw(pkg, eng, none.data_ptr(), 0, keys.data_ptr(), zero.data_ptr(), h, w, [(0, 0, 254, 0), (3, 0, 10, 0)], out=out.data_ptr(),
              lakes=lakes.data_ptr(), cap=4, host=host)
    torch.cuda.synchronize()
    assert rc == 0 and (out == 0).all() and host[0].value == 0 and host[1].tolist() == [0, 0, 0] and host[2].tolist() == [h * w, h * w]
    # no pixel
    host = _host_arrays(1)
    rc = _raw(pkg, eng, tree.data_ptr(), f.n_seeds, None, None, 0, 52, [(0, 0, 254, 0)], out=out.data_ptr(), lakes=lakes.data_ptr(), cap=4, host=host)
    assert rc == 0 and host[0].value == 0 and host[1].tolist() == [0, 0] and host[2].tolist() == [0]
    assert (out == 0).all() and (lakes == FILL).all()
    got = eng.tree_cut(tree, keys[:0], labels[:0], [pkg.Cut()], want_lakes=True)
    assert tuple(got[0].shape) == (1, 0, 52) and got[1].shape[0] == 0 and got[3].tolist() == [0]
    # no cut: nothing runs, nothing is written
    out.fill_(FILL)
    host = _host_arrays(1)
    rc = _raw(pkg, eng, tree.data_ptr(), f.n_seeds, keys.data_ptr(), labels.data_ptr(), h, w, [], out=out.data_ptr(), lakes=lakes.data_ptr(), cap=4,
              host=host)
    torch.cuda.synchronize()
    assert rc == 0 and (out == FILL).all() and host[0].value == 77 and (host[1] == 77).all()


def test_lists_only_planes_only_and_capacity(pkg, eng):
    import torch
    f, tree, keys, labels = _flood(eng, "random48x52")
    h, w = f.shape
    cuts = [tc.Cut(min_area=16), tc.Cut(min_leaves=3, show_level=100)]
    raw = [c.key() for c in cuts]
    rec, offs, hid = tc.expected_lists([f.cut(c) for c in cuts], f.n_seeds)
    total = rec.shape[0]
    # lists only
    lakes = torch.full((total + 2, 2), FILL, dtype=torch.int64, device=eng.device)
    host = _host_arrays(2)
    rc = _raw(pkg, eng, tree.data_ptr(), f.n_seeds, keys.data_ptr(), labels.data_ptr(), h, w, raw, lakes=lakes.data_ptr(), cap=total + 2, host=host)
    torch.cuda.synchronize()
    got = lakes.cpu().numpy().view(np.uint64)
    assert rc == 0 and host[0].value == total and (host[1] == offs).all() and (host[2] == hid).all()
    assert (got[:total] == rec).all() and (got[total:] == np.uint64(FILL)).all()
    # planes only: the three host pointers may be null
    out = torch.full((2, h, w), FILL, dtype=torch.int32, device=eng.device)
    rc = _raw(pkg, eng, tree.data_ptr(), f.n_seeds, keys.data_ptr(), labels.data_ptr(), h, w, raw, out=out.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    _compare(f, cuts, out.cpu().numpy().view(np.uint32))
    # one record short, then with the count it reported
    lakes.fill_(FILL)
    host = _host_arrays(2)
    rc = _raw(pkg, eng, tree.data_ptr(), f.n_seeds, keys.data_ptr(), labels.data_ptr(), h, w, raw, lakes=lakes.data_ptr(), cap=total - 1, host=host)
    torch.cuda.synchronize()
    assert rc == pkg._ffi.WS_ERR_CAPACITY and host[0].value == total
    host2 = _host_arrays(2)
    rc = _raw(pkg, eng, tree.data_ptr(), f.n_seeds, keys.data_ptr(), labels.data_ptr(), h, w, raw, lakes=lakes.data_ptr(), cap=host[0].value, host=host2)
    torch.cuda.synchronize()
    assert rc == 0 and host2[0].value == total and (lakes.cpu().numpy().view(np.uint64)[:total] == rec).all()


# ---- refusals: checks of the validation pass, which reads in bounds by construction; none of these reaches a walk --------------------

def _bad_trees(f):
    """(what, records) -- the tree of the case with ONE record spoilt."""
    dead = np.flatnonzero((f.death != tc.ALIVE) & (np.arange(f.death.size) > 1))
    both = [c for c in dead if f.death[f.parent[c]] != tc.ALIVE]      # a dying colour whose parent dies too
    c, d = int(dead[len(dead) // 2]), int(both[0])
    out = []
    for what, (col, field, value) in (("parent == c", (c, 0, c)), ("parent > c", (c, 0, c + 1)), ("parent > n_seeds", (c, 0, f.n_seeds + 5)),
                                      ("parent dies no later", (d, 1, int(f.death[f.parent[d]]))), ("death level 300", (c, 1, 300)),
                                      ("alive with a parent", (int(np.flatnonzero(f.death[1:] == tc.ALIVE)[0]) + 1, 0, 1))):
        t = f.tree.copy()
        t[col, field] = value
        out.append((what, t))
    return out


def test_refusals_leave_everything_untouched(pkg, eng):
    import torch
    f, tree, keys, labels = _flood(eng, "random48x52")
    h, w = f.shape
    ns, BAD = f.n_seeds, pkg._ffi.WS_ERR_BAD_ARG
    out = torch.full((1, h, w), FILL, dtype=torch.int32, device=eng.device)
    lakes = torch.full((ns, 2), FILL, dtype=torch.int64, device=eng.device)
    good = [(4, 0, 254, 0)]

    def refused(what, **kw):
        host = _host_arrays(1)
        args = dict(tree=tree.data_ptr(), ns=ns, keys=keys.data_ptr(), labels=labels.data_ptr(), h=h, w=w, cuts=good, out=out.data_ptr(),
                    lakes=lakes.data_ptr(), cap=ns, host=host)
        args.update(kw)
        rc = _raw(pkg, eng, **args)
        torch.cuda.synchronize()
        assert rc == BAD, (what, rc)
        assert (out == FILL).all() and (lakes == FILL).all(), what
        if args["host"] is host:
            assert host[0].value == 77 and (host[1] == 77).all() and (host[2] == 77).all(), what
        # the context is usable: a good call follows
        _compare(f, [tc.Cut(min_area=4)], eng.tree_cut(tree, keys, labels, [pkg.Cut(min_area=4)]).cpu().numpy().view(np.uint32), tag=what)

    for what, rec in _bad_trees(f):
        t = torch.from_numpy(rec.view(np.int32)).to(eng.device)
        refused(what, tree=t.data_ptr())
    refused("reserved", cuts=[(4, 0, 254, 0, 0, 1)])
    refused("show_level 255", cuts=[(4, 0, 255, 0)])
    refused("merge_level 255", cuts=[(4, 0, 254, 255)])
    refused("d_out is d_keys", out=keys.data_ptr())
    refused("d_out is d_seg_labels", out=labels.data_ptr())
    refused("short plane_stride", stride=h * w - 1)
    refused("no output", out=None, lakes=None)
    refused("null tree", tree=None)
    refused("null keys", keys=None)
    refused("null host arrays", host=None)
    assert (keys.cpu().numpy().view(np.uint32) >> 24 == f.keys32() >> 24).all() and (labels.cpu().numpy().view(np.uint32) == f.seg).all()


def test_label_above_n_seeds_is_reported_after_the_run(pkg, eng):
    import torch
    f, tree, keys, labels = _flood(eng, "random48x52")
    h, w = f.shape
    spoilt = labels.clone()
    spoilt[h // 2, w // 2] = f.n_seeds + 1
    out = torch.empty((1, h, w), dtype=torch.int32, device=eng.device)
    rc = _raw(pkg, eng, tree.data_ptr(), f.n_seeds, keys.data_ptr(), spoilt.data_ptr(), h, w, [(0, 0, 254, 0)], out=out.data_ptr())
    torch.cuda.synchronize()
    assert rc == pkg._ffi.WS_ERR_BAD_ARG
    _compare(f, [tc.Cut()], eng.tree_cut(tree, keys, labels, [pkg.Cut()]).cpu().numpy().view(np.uint32))


def test_context_with_a_begun_transform_refuses(pkg, eng):
    import torch
    f, tree, keys, labels = _flood(eng, "random48x52")
    h, w = f.shape
    t_img = torch.from_numpy(f.img).to(eng.device)
    t_seeds = torch.from_numpy(f.seeds.astype(np.int32)).to(eng.device)
    seg = torch.empty((h, w), dtype=torch.int32, device=eng.device)
    out = torch.full((1, h, w), FILL, dtype=torch.int32, device=eng.device)
    eng.segment_begin(t_img, t_seeds, seg)
    try:
        rc = _raw(pkg, eng, tree.data_ptr(), f.n_seeds, keys.data_ptr(), labels.data_ptr(), h, w, [(0, 0, 254, 0)], out=out.data_ptr())
    finally:
        eng.segment_end()
    torch.cuda.synchronize()
    assert rc == pkg._ffi.WS_ERR_BAD_ARG and (out == FILL).all()


# ---- the other roads to the same planes ---------------------------------------------------------------------------------------------

def test_round_trip_with_merge_tree_from_arrival(pkg, eng):
    import torch
    f = tc.field("random40x37")
    t_img = torch.from_numpy(f.img).to(eng.device)
    t_seeds = torch.from_numpy(f.seeds.astype(np.int32)).to(eng.device)
    labels = eng.segment(t_img, t_seeds, max_level=f.max_level)
    keys = eng.last_arrival()      # (ws_copy_last_arrival_device)
    tree = eng.merge_tree_from_arrival(keys, labels, f.n_seeds, max_level=f.max_level)
    planes, lakes, offsets, hidden = eng.tree_cut(tree, keys, labels, _pcuts(pkg, tc.MIXED_CUTS), want_lakes=True)
    torch.cuda.synchronize()
    _compare(f, tc.MIXED_CUTS, planes.cpu().numpy().view(np.uint32), lakes.cpu().numpy().view(np.uint64), offsets, hidden)


@pytest.mark.parametrize("name", ["random48x52", "random40x37_edge", "random40x37_edge_shift"])
def test_host_form(pkg, name):
    f = tc.field(name)
    cuts = tc.RANDOM_CUTS if name == "random48x52" else tc.MIXED_CUTS
    b = pkg.TransformBuilder.new().set_max_water_lvl(f.max_level)
    if f.edge:
        b.enable_edge_correction()
    if f.seed_shift:
        b.shift_seeds_into_padded_plane()
    ws = b.build_merging()
    planes, tree, (lakes, offsets, hidden) = ws.merge_tree_cut(f.img, f.seeds, _pcuts(pkg, cuts), want_tree=True, want_lakes=True)
    assert planes.dtype == np.uint64 and planes.shape == (len(cuts),) + f.shape
    got = np.stack([tree.parent, tree.death_level, tree.area, tree.n_leaves], axis=1)
    assert (got == f.tree).all()
    _compare(f, cuts, planes, lakes, offsets, hidden, tag="host")
    only = ws.merge_tree_cut(f.img, f.seeds, _pcuts(pkg, cuts[:2]))
    _compare(f, cuts[:2], only, tag="host planes only")
    with pytest.raises(ValueError):
        ws.merge_tree_cut(f.img, f.seeds, [])
