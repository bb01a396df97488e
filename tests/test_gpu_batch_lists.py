"""transform_to_list of a cube of slices in one call (ws_transform_to_list_batch(_device)) and the merging final labels of a
cube (ws_merge_batch_device), on the GPU: per (slice, level) against the CPU oracle's lake sizes, at size against the
slice-by-slice device calls on the same context, and the stack's own guarantees (it is taken, capacity protocol, context reuse)."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import oracle_lib as ol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


def _engine(pkg):
    return importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


def _seed_lists(imgs, shuffle_slice=None):
    """The slices' own minima, except: slice 1 has no seed, slice 2 a single one; `shuffle_slice`'s list is shuffled."""
    lists = [np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2) for im in imgs]
    lists[1] = lists[1][:0]
    lists[2] = lists[2][:1]
    if shuffle_slice is not None:
        lists[shuffle_slice] = lists[shuffle_slice][np.random.default_rng(5).permutation(len(lists[shuffle_slice]))]
    return lists


def _device_seeds(torch, eng, lists):
    flat = np.concatenate(lists, axis=0) if sum(len(l) for l in lists) else np.zeros((0, 2), np.int64)
    offs = [0] + list(np.cumsum([len(l) for l in lists]))
    return torch.from_numpy(flat.astype(np.int32)).to(eng.device).contiguous(), offs


def _oracle(img, seeds, merging, max_level, edge):
    want = []
    hook = lambda l, m, i, c: want.append(ol.find_lake_sizes(c))
    s = [tuple(map(int, p)) for p in seeds]
    if merging:
        ol.merge_arrival(img, s, max_level=max_level, edge=edge, hook=hook)
    else:
        ol.segment(img, s, max_level=max_level, edge=edge, hook=hook)
    return want


def _check_slice_vs_oracle(rec, offsets, unc, k, levels, want, tag):
    for lvl, w in enumerate(want):
        b = k * levels + lvl
        r = rec[int(offsets[b]):int(offsets[b + 1])]
        nz = np.nonzero(w[1:])[0] + 1
        assert unc[b] == w[0], (tag, k, lvl, int(unc[b]), int(w[0]))
        assert (np.sort(r[:, 0]) == nz).all() and (r[np.argsort(r[:, 0]), 1] == w[nz]).all(), (tag, k, lvl)


SHAPES = [((6, 128, 96), False), ((6, 126, 94), True),      # stack: the plane (padded with edge correction) is 128 x 96
          ((5, 130, 98), False), ((5, 130, 98), True)]      # no stack: w' % 4 != 0


@pytest.mark.parametrize("merging", [True, False])
@pytest.mark.parametrize("max_level", [254, 90])
@pytest.mark.parametrize("shape,edge", SHAPES)
def test_batch_lists_match_oracle_per_slice(pkg, torch, merging, max_level, shape, edge):
    s, h, w = shape
    imgs = [cases.field(h, w, 100 + 7 * k) for k in range(s)]
    levels = max_level + 1
    for shuffle in (None, 4):      # the slices' own sorted minima, then a shuffled list (the loop takes that batch)
        eng = _engine(pkg)
        lists = _seed_lists(imgs, shuffle)
        seeds, offs = _device_seeds(torch, eng, lists)
        cube = torch.from_numpy(np.stack(imgs)).to(eng.device).contiguous()
        lakes, offsets, unc = eng.transform_to_list_batch(cube, seeds, offs, merging=merging, max_level=max_level, edge=edge)
        rec = lakes.cpu().numpy()
        assert len(offsets) == s * levels + 1 and int(offsets[-1]) == len(rec) and (np.diff(offsets.astype(np.int64)) >= 0).all()
        for k in range(s):
            _check_slice_vs_oracle(rec, offsets, unc, k, levels, _oracle(imgs[k], lists[k], merging, max_level, edge),
                                   (shape, edge, merging, max_level, shuffle))


def _keys(torch, lakes, offsets, k, levels):
    """Slice k's records as one sorted key tensor (level, colour, area) on the device: equal keys = equal (level, record) sets."""
    lo, hi = int(offsets[k * levels]), int(offsets[(k + 1) * levels])
    counts = torch.from_numpy(np.diff(offsets[k * levels:(k + 1) * levels + 1].astype(np.int64))).to(lakes.device)
    lvl = torch.repeat_interleave(torch.arange(levels, device=lakes.device, dtype=torch.int64), counts)
    r = lakes[lo:hi]
    return torch.sort((lvl << 56) | (r[:, 0] << 28) | r[:, 1]).values


@pytest.mark.parametrize("kind", ["random", "smooth"])
def test_batch_lists_at_size_equal_slice_calls_and_stack_is_taken(pkg, torch, kind):
    s, h, w = 16, 1024, 1024
    eng = _engine(pkg)
    imgs = [cases.field(h, w, 300 + k) if kind == "random" else cases.smooth_field(h, w, 300 + k) for k in range(s)]
    cube = torch.from_numpy(np.stack(imgs)).to(eng.device).contiguous()
    lists = [eng.find_local_minima(cube[k]) for k in range(s)]
    offs = [0] + list(np.cumsum([int(l.shape[0]) for l in lists]))
    seeds = torch.cat(lists).contiguous()
    levels = 255
    for merging in (True, False):
        lakes, offsets, unc = eng.transform_to_list_batch(cube, seeds, offs, merging=merging)
        batch_relax = eng.stats()["launches_relax"]
        loop_relax = 0
        for k in range(s):
            one, off1, unc1 = eng.transform_to_list(cube[k], lists[k], merging=merging)
            loop_relax += eng.stats()["launches_relax"]
            b = k * levels
            assert (np.diff(offsets[b:b + levels + 1].astype(np.int64)) == np.diff(off1.astype(np.int64))).all(), (kind, merging, k)
            assert (unc[b:b + levels] == unc1).all(), (kind, merging, k)
            one_keys = _keys(torch, one, off1, 0, levels)
            assert torch.equal(_keys(torch, lakes, offsets, k, levels), one_keys), (kind, merging, k)
            del one, one_keys
        assert batch_relax < loop_relax, (kind, merging, batch_relax, loop_relax)      # one stacked flood, not sixteen


def test_batch_lists_capacity_protocol(pkg, torch):
    eng = _engine(pkg)
    s, h, w = 4, 128, 96
    imgs = [cases.field(h, w, 500 + k) for k in range(s)]
    cube = torch.from_numpy(np.stack(imgs)).to(eng.device).contiguous()
    lists = [np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2) for im in imgs]
    seeds, offs = _device_seeds(torch, eng, lists)
    full, offsets, unc = eng.transform_to_list_batch(cube, seeds, offs, merging=True)
    total = full.shape[0]
    L = pkg._ffi.lib()
    opt = eng.options(254, False)
    c_offs = (ctypes.c_size_t * (s + 1))(*[int(x) for x in offs])
    buf = torch.empty((total, 2), dtype=torch.int64, device=eng.device)
    o2 = np.zeros(s * 255 + 1, dtype=np.uint64)
    u2 = np.zeros(s * 255, dtype=np.uint64)
    n = ctypes.c_size_t(0)
    failed = ctypes.c_size_t(7)
    rc = L.ws_transform_to_list_batch_device(eng.ctx.handle, 1, cube.data_ptr(), s, h, w, w, h * w, seeds.data_ptr(), c_offs,
                                             ctypes.byref(opt), buf.data_ptr(), total - 1, ctypes.byref(n), o2.ctypes.data, u2.ctypes.data,
                                             ctypes.byref(failed))
    assert rc == pkg._ffi.WS_ERR_CAPACITY and n.value == total
    rc = L.ws_transform_to_list_batch_device(eng.ctx.handle, 1, cube.data_ptr(), s, h, w, w, h * w, seeds.data_ptr(), c_offs,
                                             ctypes.byref(opt), buf.data_ptr(), total, ctypes.byref(n), o2.ctypes.data, u2.ctypes.data,
                                             ctypes.byref(failed))
    assert rc == 0 and n.value == total and failed.value == 0
    assert (o2 == offsets).all() and (u2 == unc).all()
    for k in range(s):
        assert torch.equal(_keys(torch, buf, o2, k, 255), _keys(torch, full, offsets, k, 255))
    # argument checks with a live context
    bad = (ctypes.c_size_t * (s + 1))(0, 5, 3, 9, 12)
    assert L.ws_transform_to_list_batch_device(eng.ctx.handle, 1, cube.data_ptr(), s, h, w, w, h * w, seeds.data_ptr(), bad,
                                               ctypes.byref(opt), buf.data_ptr(), total, ctypes.byref(n), o2.ctypes.data, u2.ctypes.data,
                                               None) == pkg._ffi.WS_ERR_BAD_ARG
    assert L.ws_transform_to_list_batch_device(eng.ctx.handle, 1, cube.data_ptr(), s, h, w, w, h * w - 1, seeds.data_ptr(), c_offs,
                                               ctypes.byref(opt), buf.data_ptr(), total, ctypes.byref(n), o2.ctypes.data, u2.ctypes.data,
                                               None) == pkg._ffi.WS_ERR_BAD_ARG


def test_batch_and_single_calls_alternate_on_one_context(pkg, torch):
    # the per-level loop of a repeated call is replayed as hipGraphs: a batch (over the stack) and a single call (over one
    # slice) must never replay each other's
    eng = _engine(pkg)
    s, h, w = 4, 128, 96
    imgs = [cases.field(h, w, 600 + k) for k in range(s)]
    lists = [np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2) for im in imgs]
    cube = torch.from_numpy(np.stack(imgs)).to(eng.device).contiguous()
    seeds, offs = _device_seeds(torch, eng, lists)
    want = [_oracle(imgs[k], lists[k], True, 254, False) for k in range(s)]
    for rep in range(3):
        lakes, offsets, unc = eng.transform_to_list_batch(cube, seeds, offs, merging=True)
        rec = lakes.cpu().numpy()
        for k in range(s):
            _check_slice_vs_oracle(rec, offsets, unc, k, 255, want[k], ("batch", rep))
        p = ctypes.c_void_p()
        hh, ww = ctypes.c_size_t(), ctypes.c_size_t()
        assert pkg._ffi.lib().ws_last_arrival_device(eng.ctx.handle, ctypes.byref(p), ctypes.byref(hh), ctypes.byref(ww)) == pkg._ffi.WS_ERR_UNSUPPORTED
        k = rep % s
        one, off1, unc1 = eng.transform_to_list(cube[k], seeds[int(offs[k]):int(offs[k + 1])], merging=True)
        _check_slice_vs_oracle(one.cpu().numpy(), off1, unc1, 0, 255, want[k], ("single", rep))


def test_merge_batch_equals_slice_calls_and_oracle(pkg, torch):
    eng = _engine(pkg)
    s, h, w = 8, 512, 512
    imgs = [cases.field(h, w, 700 + k) if k % 2 else cases.smooth_field(h, w, 700 + k) for k in range(s)]
    cube = torch.from_numpy(np.stack(imgs)).to(eng.device).contiguous()
    lists = [eng.find_local_minima(cube[k]) for k in range(s)]
    offs = [0] + list(np.cumsum([int(l.shape[0]) for l in lists]))
    seeds = torch.cat(lists).contiguous()
    got = eng.merge_batch(cube, seeds, offs)
    batch_relax = eng.stats()["launches_relax"]
    loop_relax = 0
    for k in range(s):
        one = eng.merge(cube[k], lists[k])
        loop_relax += eng.stats()["launches_relax"]
        assert torch.equal(got[k], one), k
    assert batch_relax < loop_relax
    # small, against the canonical oracle labels: stack with edge correction and a seedless slice, and a shape that does not stack
    for (n, hh, ww), edge in (((5, 126, 94), True), ((5, 128, 96), False), ((4, 130, 98), False)):
        small = [cases.field(hh, ww, 800 + k) for k in range(n)]
        sl = _seed_lists(small)
        sd, so = _device_seeds(torch, eng, sl)
        cb = torch.from_numpy(np.stack(small)).to(eng.device).contiguous()
        out = eng.merge_batch(cb, sd, so, max_level=120, edge=edge).cpu().numpy().astype(np.uint32)
        for k in range(n):
            want = ol.merge_arrival(small[k], [tuple(map(int, p)) for p in sl[k]], max_level=120, edge=edge)
            assert (out[k].astype(np.uint64) == want).all(), ((n, hh, ww), edge, k)


@pytest.mark.parametrize("merging", [True, False])
def test_host_cube_lists_equal_slice_by_slice_sparse(pkg, merging):
    s, h, w = 5, 192, 160
    cube = np.stack([cases.field(h, w, 900 + k) for k in range(s)])
    b = pkg.TransformBuilder.new().set_max_water_lvl(200)
    ws = b.build_merging() if merging else b.build_segmenting()
    got, counts = ws.transform_to_list_cube(cube)
    assert len(got) == s
    for k in range(s):
        mins = ws.find_local_minima(cube[k])
        assert counts[k] == len(mins)
        want = ws.transform_to_list_sparse(cube[k], mins)
        assert len(got[k]) == len(want) == 201
        for (lvl, unc, cols, areas), (wl, wunc, wcols, wareas) in zip(got[k], want):
            assert lvl == wl and unc == wunc, (k, lvl)
            assert (np.sort(cols) == np.sort(wcols)).all() and (areas[np.argsort(cols)] == wareas[np.argsort(wcols)]).all(), (k, lvl)
    # the same with the seed lists given
    given = ws.transform_to_list_cube(cube, seeds=[ws.find_local_minima(cube[k]) for k in range(s)])
    for k in range(s):
        for (lvl, unc, cols, areas), (_, unc2, cols2, areas2) in zip(got[k], given[k]):
            assert unc == unc2 and (np.sort(cols) == np.sort(cols2)).all(), (k, lvl)
