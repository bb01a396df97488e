"""merge_tree and the lake catalogue from the planes of a transform that has already run (ws_merge_tree_from_arrival_device),
-m gpu: bit for bit against ws_merge_tree_device / ws_merge_tree_stats_device on the image and the seed list, and both against
the records derived from the CPU oracle's per-level planes (tests/merge_tree_ref.py, tests/lake_stats_ref.py).  The form gets
no seed list: tests/test_tree_from_arrival_cpu.py proves on the oracle that stamp 0 marks the seed pixels.  Every comparison is
on integers and exact."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import lake_stats_batch_cases as lbc
import lake_stats_ref as ls
import merge_tree_ref as mt
import merging_cases as mc
import oracle_lib as ol

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


def _to_dev(eng, img, seeds):
    import torch
    t_img = torch.from_numpy(np.ascontiguousarray(img)).to(eng.device)
    t_seeds = torch.from_numpy(np.asarray(seeds, dtype=np.int64).reshape(-1, 2).astype(np.int32)).to(eng.device)
    return t_img, t_seeds


def _w_dev(eng, wt):
    """A u8 plane as it is, a u16 plane as its int16 bits."""
    import torch
    wt = np.ascontiguousarray(wt)
    return torch.from_numpy(wt if wt.dtype == np.uint8 else wt.view(np.int16)).to(eng.device)


def _weights(shape, seed):
    """A u8 and a u16 plane, neither a function of the image; the u16 one holds 0 and 65535 several times (ties at the peak)."""
    rng = np.random.default_rng(1000 + seed)
    u8 = rng.integers(0, 256, shape, dtype=np.uint8)
    u16 = rng.integers(0, 65536, shape, dtype=np.uint16)
    flat = u16.reshape(-1)
    where = rng.permutation(flat.size)
    flat[where[:max(flat.size // 50, 2)]] = 65535
    flat[where[-max(flat.size // 50, 2):]] = 0
    return [("u8", u8), ("u16", u16)]


def _padded(wt, edge):
    """The weight plane of the (padded) label plane: under edge correction a ring of weight 0 around it."""
    return np.ascontiguousarray(np.pad(wt, 1)) if edge else wt


def _np(t):
    return t.cpu().numpy()


def _planes(eng, t_img, t_seeds, **kw):
    """The stamps and labels a segmenting transform leaves: copies, so that later transforms on the context do not change them."""
    labels = eng.segment(t_img, t_seeds, **kw).clone()
    return eng.last_arrival().clone(), labels


def _check(eng, img, seeds, max_level=254, edge=False, seed_shift=False, tag=None, oracle=True):
    import torch
    img = np.ascontiguousarray(img)
    seeds = np.asarray(seeds, dtype=np.int64).reshape(-1, 2)
    t_img, t_seeds = _to_dev(eng, img, seeds)
    kw = dict(max_level=max_level, edge=edge, seed_shift=seed_shift)
    keys, labels = _planes(eng, t_img, t_seeds, **kw)
    n = len(seeds)
    want_tree = _np(eng.merge_tree(t_img, t_seeds, **kw)).view(np.uint32)
    got_tree = _np(eng.merge_tree_from_arrival(keys, labels, n, max_level=max_level)).view(np.uint32)
    assert (got_tree == want_tree).all(), (tag, "tree", np.flatnonzero((got_tree != want_tree).any(axis=1))[:8])
    if oracle:      # the oracle's planes once per input
        planes, ps = mt.oracle_planes(img, seeds, max_level, edge, seed_shift)
        parent, death, area, leaves, _, ex = mt.tree_from_planes(planes, ps)
        assert (want_tree == np.stack([parent, death, area, leaves], axis=1)).all(), (tag, "oracle tree")
    for name, wt in _weights(img.shape, 3):
        ref_tree, ref = eng.merge_tree_stats(t_img, t_seeds, weights=_w_dev(eng, wt), **kw)
        tree, raw = eng.merge_tree_from_arrival(keys, labels, n, max_level=max_level, weights=_w_dev(eng, _padded(wt, edge)), want_stats=True)
        torch.cuda.synchronize()
        assert (_np(tree).view(np.uint32) == want_tree).all() and (_np(ref_tree).view(np.uint32) == want_tree).all(), (tag, name)
        got, ref = ls.from_raw(_np(raw)), ls.from_raw(_np(ref))
        assert ls.mismatch(got, ref) is None, (tag, name, ls.mismatch(got, ref))
        if oracle:
            o_rec = ls.stats_from_planes(planes, ps, ls.plane_weights(img, wt, edge), death, ex)
            assert ls.mismatch(got, o_rec) is None, (tag, name, "oracle", ls.mismatch(got, o_rec))
    return keys, labels, want_tree


FIELD = cases.field(210, 330, 8)


@pytest.mark.parametrize("edge,shift", [(False, False), (True, True)])
def test_random_field(eng, edge, shift):
    _check(eng, FIELD, ol.find_local_minima(FIELD), edge=edge, seed_shift=shift)


def test_width_not_a_multiple_of_four(eng):
    img = cases.field(97, 131, 5)
    _check(eng, img, ol.find_local_minima(img))
    _check(eng, img, ol.find_local_minima(img), edge=True)      # 133 wide padded


def test_duplicates_and_a_shuffled_list(eng):
    rng = np.random.default_rng(77)
    img = mc.make_field("few", 90, 132, rng)
    for form in ("repeats", "shuffled", "borders"):
        _check(eng, img, mc.make_seeds(form, 90, 132, 90 * 132 // 30, rng), tag=form)


def test_the_deep_chain(eng):
    case = mc.staircase()      # 254 hooks deep: colour c dies at level 255 - c into c - 1
    _, _, tree = _check(eng, case.img, case.seeds, tag="staircase")
    depth, c = 0, len(tree) - 1
    while tree[c, 1] != 0xFFFFFFFF:
        c, depth = int(tree[c, 0]), depth + 1
    assert depth == 254


def test_a_death_at_level_zero(eng):
    imgs, lists, dying = lbc.level_zero_death_case()
    for k, colour in dying:
        _, _, tree = _check(eng, imgs[k], lists[k], tag=("level0", k))
        assert tree[colour, 1] == 0 and tree[colour, 2] == 1 and tree[colour, 3] == 1


def test_max_level_40(eng):
    img = cases.field(120, 140, 12)
    _check(eng, img, ol.find_local_minima(img), max_level=40)
    _check(eng, cases.smooth_field(90, 112, 8), ol.find_local_minima(cases.smooth_field(90, 112, 8)), max_level=40, edge=True, seed_shift=True)


@pytest.mark.parametrize("shape", [(64, 96), (61, 83)])
def test_planes_as_views_off_16_byte_alignment(eng, shape):
    """The planes one u32 into larger buffers: every kernel that reads them takes its scalar path.  (64 x 96: a width whose
    aligned planes take the 16-byte loads everywhere.)"""
    import torch
    img = cases.field(*shape, 21)
    seeds = np.asarray(ol.find_local_minima(img), dtype=np.int64).reshape(-1, 2)
    t_img, t_seeds = _to_dev(eng, img, seeds)
    keys, labels = _planes(eng, t_img, t_seeds)
    n_px = img.size
    big_k = torch.full((n_px + 9,), -1, dtype=torch.int32, device=eng.device)
    big_l = torch.full((n_px + 9,), -1, dtype=torch.int32, device=eng.device)
    big_k[1:1 + n_px] = keys.reshape(-1)
    big_l[5:5 + n_px] = labels.reshape(-1)
    vk, vl = big_k[1:1 + n_px].view(shape), big_l[5:5 + n_px].view(shape)
    assert vk.data_ptr() % 16 == 4 and vl.data_ptr() % 16 == 4
    wt = _weights(shape, 4)[1][1]
    want_tree, want = eng.merge_tree_from_arrival(keys, labels, len(seeds), weights=_w_dev(eng, wt), want_stats=True)
    tree, raw = eng.merge_tree_from_arrival(vk, vl, len(seeds), weights=_w_dev(eng, wt), want_stats=True)
    ref_tree, ref = eng.merge_tree_stats(t_img, t_seeds, weights=_w_dev(eng, wt))
    torch.cuda.synchronize()
    assert (_np(tree) == _np(want_tree)).all() and (_np(tree) == _np(ref_tree)).all()
    assert (_np(raw) == _np(want)).all() and (_np(raw) == _np(ref)).all()
    # only keys off alignment, only labels off alignment
    for a, b in ((vk, labels), (keys, vl)):
        t2, r2 = eng.merge_tree_from_arrival(a, b, len(seeds), weights=_w_dev(eng, wt), want_stats=True)
        assert (_np(t2) == _np(ref_tree)).all() and (_np(r2) == _np(ref)).all()


def test_alternating_calls_on_one_context(pkg, eng):
    """The arrival form twice on the same planes (the second replays the level loop's graphs), on other planes of the same shape,
    between the image form and the lists' arrival form: every result equals its first."""
    import torch
    L, ffi = pkg._ffi.lib(), pkg._ffi
    shape = (96, 128)
    a, b = cases.field(*shape, 41), cases.field(*shape, 42)
    sa = np.asarray(ol.find_local_minima(a), dtype=np.int64).reshape(-1, 2)
    sb = np.asarray(ol.find_local_minima(b), dtype=np.int64).reshape(-1, 2)[:len(sa)]
    sa = sa[:len(sb)]      # the same number of colours: the two calls differ in their planes alone
    n = len(sa)
    (ta, tsa), (tb, tsb) = _to_dev(eng, a, sa), _to_dev(eng, b, sb)
    ka, la = _planes(eng, ta, tsa)
    kb, lb = _planes(eng, tb, tsb)
    wa, wb = _w_dev(eng, _weights(shape, 41)[1][1]), _w_dev(eng, _weights(shape, 42)[1][1])
    want_a = [_np(x).copy() for x in eng.merge_tree_stats(ta, tsa, weights=wa)]
    want_b = [_np(x).copy() for x in eng.merge_tree_stats(tb, tsb, weights=wb)]
    assert not (want_a[0] == want_b[0]).all()

    def arrival(k, l, w):
        return [_np(x).copy() for x in eng.merge_tree_from_arrival(k, l, n, weights=w, want_stats=True)]

    def lists():
        cap = 256 * (n + 1)
        rec = torch.zeros((cap, 2), dtype=torch.int64, device=eng.device)
        n_lakes = ctypes.c_size_t(0)
        off, unc = np.zeros(256, dtype=np.uint64), np.zeros(255, dtype=np.uint64)
        opt = ffi.Options(254)
        eng.ctx.check(L.ws_lists_from_arrival_device(eng.ctx.handle, 1, ka.data_ptr(), la.data_ptr(), shape[0], shape[1], n, ctypes.byref(opt),
                                                     rec.data_ptr(), cap, ctypes.byref(n_lakes), off.ctypes.data, unc.ctypes.data))
        return n_lakes.value, off.copy(), unc.copy()

    first = arrival(ka, la, wa)
    assert eng.stats()["graph_launches"] == 0
    second = arrival(ka, la, wa)
    assert eng.stats()["graph_launches"] == 16      # 255 levels in groups of 16: the same planes replay
    other = arrival(kb, lb, wb)
    assert eng.stats()["graph_launches"] == 0       # other planes of the same shape and colour count must not
    image_form = [_np(x).copy() for x in eng.merge_tree_stats(ta, tsa, weights=wa)]
    lists_1 = lists()
    again = arrival(ka, la, wa)
    lists_2 = lists()
    for got in (first, second, again, image_form):
        assert (got[0] == want_a[0]).all() and (got[1] == want_a[1]).all()
    assert (other[0] == want_b[0]).all() and (other[1] == want_b[1]).all()
    assert lists_1[0] == lists_2[0] and (lists_1[1] == lists_2[1]).all() and (lists_1[2] == lists_2[2]).all()


def test_the_stamp_report_is_left_alone(eng):
    import torch
    img, other = cases.field(70, 88, 51), cases.field(70, 88, 52)
    t_img, t_seeds = _to_dev(eng, img, ol.find_local_minima(img))
    keys, labels = _planes(eng, t_img, t_seeds)
    t_other, t_os = _to_dev(eng, other, ol.find_local_minima(other))
    eng.segment(t_other, t_os)      # the context's last transform is another one now
    before = eng.last_arrival().clone()
    assert not (before == keys).all()
    eng.merge_tree_from_arrival(keys, labels, t_seeds.shape[0])
    torch.cuda.synchronize()
    assert (eng.last_arrival() == before).all()


def test_empty_inputs_write_record_zero_only(pkg, eng):
    import torch
    L, ffi = pkg._ffi.lib(), pkg._ffi
    opt = ffi.Options(254)
    img = cases.field(33, 40, 61)
    t_img, none = _to_dev(eng, img, np.zeros((0, 2), dtype=np.int64))
    keys, labels = _planes(eng, t_img, none)
    wt = _w_dev(eng, _weights(img.shape, 61)[0][1])
    ref_tree, ref = eng.merge_tree_stats(t_img, none, weights=wt)
    tree = torch.full((3, 4), 77, dtype=torch.int32, device=eng.device)
    stats = torch.full((3, 9), 77, dtype=torch.int64, device=eng.device)
    # no seeds: record 0 of both, the plane uncoloured
    eng.ctx.check(L.ws_merge_tree_from_arrival_device(eng.ctx.handle, keys.data_ptr(), labels.data_ptr(), 33, 40, 0, ctypes.byref(opt), wt.data_ptr(),
                                                      ffi.WS_DTYPES["uint8"], 40, tree.data_ptr(), stats.data_ptr()))
    torch.cuda.synchronize()
    assert (_np(tree)[0] == _np(ref_tree)[0]).all() and (_np(stats)[0] == _np(ref)[0]).all()
    assert _np(tree).view(np.uint32)[0].tolist() == [0, 0xFFFFFFFF, 33 * 40, 0]
    assert (_np(tree)[1:] == 77).all() and (_np(stats)[1:] == 77).all()
    # no pixels: record 0 only, whatever the seed count says, and the planes may be null
    tree.fill_(77)
    stats.fill_(77)
    for h, w in ((0, 7), (5, 0)):
        eng.ctx.check(L.ws_merge_tree_from_arrival_device(eng.ctx.handle, None, None, h, w, 2, ctypes.byref(opt), wt.data_ptr(), ffi.WS_DTYPES["uint8"],
                                                          max(w, 1), tree.data_ptr(), stats.data_ptr()))
        torch.cuda.synchronize()
        assert _np(tree).view(np.uint32)[0].tolist() == [0, 0xFFFFFFFF, 0, 0]
        assert ls.mismatch(ls.from_raw(_np(stats)[:1]), ls.empty_records(1)) is None
        assert (_np(tree)[1:] == 77).all() and (_np(stats)[1:] == 77).all()


def test_refusals_leave_the_outputs_untouched(pkg, eng):
    import torch
    L, ffi = pkg._ffi.lib(), pkg._ffi
    opt = ffi.Options(254)
    img = cases.field(33, 40, 62)
    seeds = ol.find_local_minima(img)
    t_img, t_seeds = _to_dev(eng, img, seeds)
    keys, labels = _planes(eng, t_img, t_seeds)
    n = t_seeds.shape[0]
    wt = _w_dev(eng, _weights(img.shape, 62)[0][1])
    tree = torch.full((n + 1, 4), 77, dtype=torch.int32, device=eng.device)
    stats = torch.full((n + 1, 9), 77, dtype=torch.int64, device=eng.device)
    u8 = ffi.WS_DTYPES["uint8"]

    def call(k, l, h, w, weight, dtype, stride, d_tree=tree, d_stats=stats, o=opt):
        return L.ws_merge_tree_from_arrival_device(eng.ctx.handle, k, l, h, w, n, ctypes.byref(o), weight, dtype, stride,
                                                   d_tree.data_ptr() if d_tree is not None else None, d_stats.data_ptr() if d_stats is not None else None)

    kp, lp, wp = keys.data_ptr(), labels.data_ptr(), wt.data_ptr()
    assert call(kp, lp, 33, 40, None, u8, 40) == ffi.WS_ERR_BAD_ARG                        # the catalogue without weights: no image here
    assert b"no image" in L.ws_last_error(eng.ctx.handle)
    assert call(kp, lp, 33, 40, wp, ffi.WS_DTYPES["float32"], 40) == ffi.WS_ERR_UNSUPPORTED      # a dtype that is no weight
    assert call(kp, lp, 33, 40, wp, u8, 39) == ffi.WS_ERR_BAD_ARG                          # a short weight stride
    assert call(None, lp, 33, 40, wp, u8, 40) == ffi.WS_ERR_BAD_ARG                        # null planes of a non-zero size
    assert call(kp, None, 33, 40, wp, u8, 40) == ffi.WS_ERR_BAD_ARG
    assert call(kp, lp, 33, 40, wp, u8, 40, d_tree=None) == ffi.WS_ERR_BAD_ARG
    assert call(kp, lp, 33, 40, wp, u8, 40, o=ffi.Options(255)) == ffi.WS_ERR_MAX_TOO_HIGH
    torch.cuda.synchronize()
    assert (_np(tree) == 77).all() and (_np(stats) == 77).all()
    # the tree alone ignores the weight arguments; and the context runs a good call after the refusals
    assert call(kp, lp, 33, 40, None, 99, 0, d_stats=None) == 0
    assert call(kp, lp, 33, 40, wp, u8, 40) == 0
    torch.cuda.synchronize()
    ref_tree, ref = eng.merge_tree_stats(t_img, t_seeds, weights=wt)
    assert (_np(tree) == _np(ref_tree)).all() and (_np(stats) == _np(ref)).all()
