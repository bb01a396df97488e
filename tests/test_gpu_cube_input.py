"""The cube front end on the GPU, -m gpu: ws_pre_processor_batch(_device) and ws_find_local_minima_batch(_device) with their numpy
and torch shims.  Every comparison is bit for bit.

  pre-processor   reference = the C oracle's pre_processor of each slice made contiguous (ol.pre_processor), never the engine; the
                  single call ws_pre_processor_device on one slice is a second witness
  minima          reference = the oracle's find_local_minima of each slice, concatenated; ws_find_local_minima_device on each slice
                  is the second witness
The cubes come from tests/cube_input_cases.py; what they are claimed to contain is proved in tests/test_cube_input_cases_cpu.py.
"""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cube_input_cases as cc
import oracle_lib as ol
import preproc_cases as pc

pytestmark = pytest.mark.gpu

GUARD = 0xA5
LEAD = 64


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def eng(pkg, torch):
    with torch.cuda.stream(torch.cuda.Stream(0)):
        yield importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


@pytest.fixture(scope="module")
def ws(pkg):
    return pkg.TransformBuilder.default().build_merging()


_WANT = {}


def _want(key, cube, mx):
    """The reference of one cube, computed once: every slice's own ol.pre_processor."""
    if key not in _WANT:
        _WANT[key] = np.stack([ol.pre_processor(np.ascontiguousarray(s), mx) for s in cube])
    return _WANT[key]


def _root(view):
    r = view
    while r.base is not None:
        r = r.base
    return r


def _to_dev(torch, eng, view):
    """The view's storage on the device; returns (tensor that owns it, device address of the view's first element)."""
    root = _root(view)
    raw = torch.from_numpy(np.ascontiguousarray(root).view(np.uint8).reshape(-1).copy()).to(eng.device)
    return raw, raw.data_ptr() + (view.ctypes.data - root.ctypes.data)


def _device_pre(pkg, torch, eng, view, mx=254, out_lead=LEAD, want_minmax=True, ctx=None):
    """ws_pre_processor_batch_device on a numpy view's storage with the view's own strides, into a window of a guard-filled buffer.
    Returns (status, cube, minmax, guards intact, failed slice)."""
    n, h, w = view.shape
    keep, ptr = _to_dev(torch, eng, view)
    ss, rs, cs = cc.element_strides(view)
    total = n * h * w
    out = torch.full((out_lead + total + LEAD,), GUARD, dtype=torch.uint8, device=eng.device)
    mm = torch.full((2 * n + 2,), -7.0, dtype=torch.float64, device=eng.device)
    failed = ctypes.c_size_t(2 ** 40)
    rc = pkg._ffi.lib().ws_pre_processor_batch_device((ctx or eng.ctx).handle, ptr, pkg._ffi.WS_DTYPES[view.dtype.name], n, h, w, ss, rs, cs, mx,
                                                      out.data_ptr() + out_lead, mm.data_ptr() if want_minmax else None, ctypes.byref(failed))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    intact = bool((got[:out_lead] == GUARD).all() and (got[out_lead + total:] == GUARD).all())
    mmh = mm.cpu().numpy()
    intact = intact and mmh[2 * n] == -7.0 and mmh[2 * n + 1] == -7.0
    return rc, got[out_lead:out_lead + total].reshape(n, h, w), mmh[:2 * n].reshape(n, 2), intact, failed.value


# ---- pre-processor ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", cc.LAYOUTS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_every_slice_count_and_plane_size(pkg, torch, eng, dtype, layout):
    """K x planes: every partial tile on both tile axes, in one layout and dtype; MAX and the output's alignment rotate through the
    combinations (test_max_values_and_alignments runs them all on the tile-edge shapes)."""
    i = 0
    for n in cc.K_SET:
        for h, w in cc.PLANES:
            mx = (1, 127, 254)[i % 3]
            lead = (LEAD, 1, 2)[(i // 3) % 3]
            i += 1
            cube = cc.preproc_cube(n, h, w, dtype)
            rc, got, mm, intact, _ = _device_pre(pkg, torch, eng, cc.lay_out(cube, layout), mx, out_lead=lead)
            assert rc == 0 and intact, (n, h, w, mx, rc)
            want = _want((dtype, n, h, w, mx, "plain"), cube, mx)
            assert (got == want).all(), (n, h, w, mx, np.argwhere(got != want)[:4])
            assert (mm == cc.seeded_minmax(cube)).all(), (n, h, w)


@pytest.mark.parametrize("layout", cc.LAYOUTS)
def test_max_values_and_alignments(pkg, torch, eng, layout):
    for dtype in ("float32", "int16"):
        for n, (h, w) in ((cc.CL_S + 1, (1, cc.CL_P + 1)), (2, (4, 64)), (cc.CL_S, (2, cc.CL_P))):
            cube = cc.preproc_cube(n, h, w, dtype)
            for mx in (1, 127, 254):
                want = _want((dtype, n, h, w, mx, "plain"), cube, mx)
                for lead in (LEAD, 1, 2, 3):      # a 4-byte aligned window takes the packed stores where h * w % 4 == 0
                    rc, got, _, intact, _ = _device_pre(pkg, torch, eng, cc.lay_out(cube, layout), mx, out_lead=lead, want_minmax=False)
                    assert rc == 0 and intact and (got == want).all(), (dtype, n, h, w, mx, lead)


@pytest.mark.parametrize("layout", cc.LAYOUTS)
def test_rounding_ramps_as_slices(pkg, torch, eng, layout):
    """The ramps on which any other order of the quantiser's operations is wrong somewhere (preproc_cases.rounding_cases)."""
    for r in pc.ROUNDING_R:
        for lo in (0, -(r // 2)):
            for dtype in ("float64", "float32", "int32") + (("uint16",) if lo == 0 else ()):
                cube = cc.rounding_cube(dtype, r, lo)
                for mx in pc.ROUNDING_MAX:
                    rc, got, _, intact, _ = _device_pre(pkg, torch, eng, cc.lay_out(cube, layout), mx, want_minmax=False)
                    assert rc == 0 and intact and (got == _want((dtype, r, lo, mx, "ramp"), cube, mx)).all(), (r, lo, dtype, mx)


@pytest.mark.parametrize("layout", cc.LAYOUTS)
@pytest.mark.parametrize("dtype", ("float64", "float32"))
def test_specials_and_degenerate_slices(pkg, torch, eng, dtype, layout):
    """NaN, +inf and -inf beside the extremes; a slice of NaN only, of zeros only and of negatives only between ordinary ones."""
    cube = cc.preproc_cube(7, 3, 43, dtype, flank=True)
    cube[1] = np.nan
    cube[3] = 0
    cube[5] = -(1 + np.arange(3 * 43) % 5).reshape(3, 43)
    rc, got, mm, intact, _ = _device_pre(pkg, torch, eng, cc.lay_out(cube, layout))
    want = _want((dtype, "specials"), cube, 254)
    assert rc == 0 and intact and (got == want).all()
    assert (got[1] == 255).all() and (got[3] == 255).all() and got[5].max() < 255
    assert (mm == cc.seeded_minmax(cube)).all() and tuple(mm[1]) == (0.0, 0.0) and tuple(mm[5]) == (-5.0, 0.0)


def test_one_slice_equals_the_single_call(pkg, torch, eng):
    for dtype in cc.DTYPES:
        cube = cc.preproc_cube(1, 5, 205, dtype)
        rc, got, _, intact, _ = _device_pre(pkg, torch, eng, cube)
        t_in = torch.from_numpy(cube).to(eng.device)
        single = eng.pre_processor(t_in, 254)
        torch.cuda.synchronize()
        assert rc == 0 and intact and (got == single.cpu().numpy()).all() and single.shape == t_in.shape
        assert (got[0] == ol.pre_processor(cube[0])).all()


def test_f64_overflow_names_the_lowest_slice(pkg, torch, eng, ws):
    ffi = pkg._ffi
    bad, near = cc.overflow_cube()
    for layout in cc.LAYOUTS:
        rc, _, mm, intact, failed = _device_pre(pkg, torch, eng, cc.lay_out(bad, layout))
        assert rc == ffi.WS_ERR_UNSUPPORTED and failed == 3 and intact
        assert b"lib.rs:1164" in ffi.lib().ws_last_error(eng.ctx.handle)
        assert (mm == cc.seeded_minmax(bad)).all()
        rc, got, _, intact, _ = _device_pre(pkg, torch, eng, cc.lay_out(near, layout))
        assert rc == 0 and intact and (got == _want("near", near, 254)).all()
        with np.errstate(over="ignore"):
            as32 = bad.astype(np.float32)      # +-inf: filtered out of the folds, no overflow
        rc, got, _, intact, _ = _device_pre(pkg, torch, eng, cc.lay_out(as32, layout))
        assert rc == 0 and intact and (got == _want("as32", as32, 254)).all()
    with pytest.raises(pkg.api.WatershedError, match="slice 3") as e:
        ws.pre_processor_cube(bad)
    assert e.value.status == ffi.WS_ERR_UNSUPPORTED
    assert (ws.pre_processor_cube(near) == _want("near", near, 254)).all()      # the next call on the context works


def test_many_thin_slices_channel_last(pkg, torch, eng):
    n = 65537
    rng = np.random.default_rng(3)
    cube = rng.integers(-300, 300, size=(n, 1, 3)).astype(np.float32)
    cube[::7, 0, 1] = np.nan
    rc, got, mm, intact, _ = _device_pre(pkg, torch, eng, cc.lay_out(cube, "channel_last"))
    assert rc == 0 and intact
    x = np.where(np.isfinite(cube), cube, 0).astype(np.float64).reshape(n, 3)
    mn, mxv = np.minimum(x.min(axis=1), 0), np.maximum(x.max(axis=1), 0)
    assert (mm[:, 0] == mn).all() and (mm[:, 1] == mxv).all()
    pick = np.r_[0:70, n - 70:n, 32760:32780, 65530:65537]
    for k in pick:
        assert (got[k] == ol.pre_processor(np.ascontiguousarray(cube[k]))).all(), k
    # every slice, by the numpy restatement of the same arithmetic (f64, same operation order)
    c64 = cube.astype(np.float64).reshape(n, 3)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.trunc(((c64 - mn[:, None]) / (mxv - mn)[:, None]) * 254.0)
    normal = np.isfinite(c64) & (np.abs(c64) >= np.finfo(np.float64).tiny)
    want = np.where(normal, q, 255).astype(np.uint8)
    assert (got.reshape(n, 3) == want).all()


def test_refusals(pkg, torch, eng):
    ffi = pkg._ffi
    L = ffi.lib()
    cube = cc.preproc_cube(2, 3, 5, "float32")
    t_in = torch.from_numpy(cube).to(eng.device)
    out = torch.full((30 + 8,), GUARD, dtype=torch.uint8, device=eng.device)
    h = eng.ctx.handle

    def call(data=t_in.data_ptr(), dtype=0, n=2, mx=254, dst=out.data_ptr()):
        return L.ws_pre_processor_batch_device(h, data, dtype, n, 3, 5, 15, 5, 1, mx, dst, None, None)

    assert call(mx=0) == ffi.WS_ERR_MAX_TOO_LOW and call(mx=255) == ffi.WS_ERR_MAX_TOO_HIGH
    assert call(dtype=6) == ffi.WS_ERR_BAD_ARG and call(dtype=-1) == ffi.WS_ERR_BAD_ARG
    assert call(data=None) == ffi.WS_ERR_BAD_ARG and call(dst=None) == ffi.WS_ERR_BAD_ARG
    assert L.ws_pre_processor_batch_device(None, t_in.data_ptr(), 0, 2, 3, 5, 15, 5, 1, 254, out.data_ptr(), None, None) == ffi.WS_ERR_BAD_ARG
    assert call(n=0, data=None, dst=None) == 0                       # nothing to do: null pointers allowed, nothing written
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all()
    host_out = np.full(30, GUARD, np.uint8)
    assert L.ws_pre_processor_batch(h, cube.ctypes.data, 0, 2, 3, 5, 15, 5, 1, 0, host_out.ctypes.data, None, None) == ffi.WS_ERR_MAX_TOO_LOW
    assert L.ws_pre_processor_batch(h, None, 0, 2, 3, 5, 15, 5, 1, 254, host_out.ctypes.data, None, None) == ffi.WS_ERR_BAD_ARG
    assert (host_out == GUARD).all()
    # a context that holds a begun transform takes neither call
    img = eng.random_field(64, 64, 1)
    seeds = eng.find_local_minima(img)
    labels = torch.empty((64, 64), dtype=torch.int32, device=eng.device)
    eng.segment_begin(img, seeds, labels)
    try:
        assert call() == ffi.WS_ERR_BAD_ARG
        offs = (ctypes.c_size_t * 3)()
        n = ctypes.c_size_t(0)
        assert L.ws_find_local_minima_batch_device(h, img.data_ptr(), 1, 64, 64, 64, 4096, None, 0, offs, ctypes.byref(n)) == ffi.WS_ERR_BAD_ARG
    finally:
        eng.segment_end()
    assert call() == 0


@pytest.mark.parametrize("axis", (0, 2))
def test_host_form_and_shims(pkg, torch, eng, ws, axis):
    for dtype in ("float32", "float64", "uint16"):
        cube = cc.preproc_cube(5, 6, 67, dtype, flank=dtype != "uint16")
        want = _want((dtype, "shim"), cube, 254)
        want127 = _want((dtype, "shim127"), cube, 127)
        store = np.ascontiguousarray(np.moveaxis(cube, 0, axis))       # axis 2: (h, w, n), the layout the reference's tests slice
        assert (ws.pre_processor_cube(store, axis=axis) == want).all()
        assert (ws.pre_processor_with_max_cube(store, 127, axis=axis) == want127).all()
        assert (ws.pre_processor_with_max_cube(np.moveaxis(cube, 0, axis)[:, ::-1], 127, axis=axis) ==
                _want((dtype, "flip", axis), np.moveaxis(np.moveaxis(cube, 0, axis)[:, ::-1], axis, 0), 127)).all()      # a negative stride: copied
        if dtype == "uint16" and not hasattr(torch, "uint16"):
            continue
        t = torch.from_numpy(store).to(eng.device)
        got, mm = eng.pre_processor_batch(t, axis=axis, want_minmax=True)
        torch.cuda.synchronize()
        assert got.shape == cube.shape and got.is_contiguous() and (got.cpu().numpy() == want).all()
        assert (mm.cpu().numpy() == cc.seeded_minmax(cube)).all()
        assert (eng.pre_processor_batch(t, axis=axis, max_value=127).cpu().numpy() == want127).all()
    # the raw host form with the strided view: one copy of the span, the view's strides
    cube = cc.preproc_cube(3, 4, 9, "int32")
    view = cc.lay_out(cube, "strided")
    ss, rs, cs = cc.element_strides(view)
    out = np.full(3 * 4 * 9 + 8, GUARD, np.uint8)
    mm = np.zeros(6)
    rc = pkg._ffi.lib().ws_pre_processor_batch(ws._ctx().handle, view.ctypes.data, pkg._ffi.WS_DTYPES["int32"], 3, 4, 9, ss, rs, cs, 254,
                                               out.ctypes.data, mm.ctypes.data, None)
    assert rc == 0 and (out[:108].reshape(3, 4, 9) == _want("host-strided", cube, 254)).all() and (out[108:] == GUARD).all()
    assert (mm.reshape(3, 2) == cc.seeded_minmax(cube)).all()


# ---- minima ------------------------------------------------------------------------------------------------------------------------

def _device_minima(pkg, torch, eng, view, cap=None, null_list=False):
    """ws_find_local_minima_batch_device on a u8 view (slices, rows, columns; unit column stride) with the view's strides.
    Returns (status, seeds (cap, 2) as the device holds them, offsets, total, guards intact)."""
    n, h, w = view.shape
    keep, ptr = _to_dev(torch, eng, view)
    ss, rs, cs = view.strides
    assert cs == 1 or w <= 1
    bound = ((max(h, 1) - 1) // 2 + 1) * ((max(w, 1) - 1) // 2 + 1) * n
    cap = bound if cap is None else cap
    out = torch.full((2 * cap + 16,), 0x5A5A5A5A, dtype=torch.int32, device=eng.device)
    offs = np.full(n + 2, 2 ** 50, dtype=np.uintp)
    total = ctypes.c_size_t(2 ** 40)
    rc = pkg._ffi.lib().ws_find_local_minima_batch_device(eng.ctx.handle, ptr, n, h, w, rs, ss, None if null_list else out.data_ptr(), cap,
                                                          offs.ctypes.data_as(pkg._ffi.szp), ctypes.byref(total))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    intact = bool((got[2 * cap:] == 0x5A5A5A5A).all()) and offs[n + 1] == 2 ** 50
    return rc, got[:2 * cap].reshape(-1, 2).astype(np.uint64), offs[:n + 1].astype(np.uint64), total.value, intact


def _check_minima(pkg, torch, eng, cube, view=None, tag=None):
    want, want_offs = cc.per_slice_minima(cube, ol.find_local_minima)
    rc, got, offs, total, intact = _device_minima(pkg, torch, eng, cube if view is None else view)
    assert rc == 0 and intact and total == len(want), (tag, rc, total, len(want))
    assert (offs == want_offs).all(), tag
    assert (got[:total] == want).all(), tag
    return want, want_offs


@pytest.mark.parametrize("name", ("border", "seedless", "lattice"))
def test_minima_of_the_proved_cubes(pkg, torch, eng, name):
    cube = {"border": cc.border_maxima_cube, "seedless": cc.seedless_cube, "lattice": cc.lattice_cube}[name]()
    want, offs = _check_minima(pkg, torch, eng, cube, tag=name)
    dev = torch.from_numpy(cube).to(eng.device)
    for k in range(cube.shape[0]):      # the single call on each slice is the second witness
        single = eng.find_local_minima(dev[k]).cpu().numpy().astype(np.uint64)
        assert (single == want[int(offs[k]):int(offs[k + 1])]).all(), (name, k)
    if name == "lattice":               # the most a cube can hold, met exactly: cap == count passes, one less does not
        count = cc.lattice_count(*cube.shape)
        rc, got, _, total, intact = _device_minima(pkg, torch, eng, cube, cap=count)
        assert rc == 0 and total == count and intact and (got == want).all()
    seeds, offsets = eng.find_local_minima_batch(dev)
    assert (seeds.cpu().numpy().astype(np.uint64) == want).all() and (offsets.astype(np.uint64) == offs).all()


@pytest.mark.parametrize("h", cc.MINIMA_H)
def test_minima_shapes(pkg, torch, eng, h):
    for w in cc.MINIMA_W:
        _check_minima(pkg, torch, eng, cc.random_cube(5, h, w, 100 * h + w), tag=(h, w))


def test_minima_unaligned_view_with_odd_strides(pkg, torch, eng):
    n, h, w = 5, 9, 33
    store = np.random.default_rng(9).integers(0, 256, size=n * ((h + 2) * 37 + 2) + 3, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(store[3:], shape=(n, h, w), strides=((h + 2) * 37 + 2, 37, 1))      # base off 4 bytes, odd strides
    assert view.ctypes.data % 4 and view.strides[0] % 2 == 1 and view.strides[1] % 2 == 1
    _check_minima(pkg, torch, eng, np.ascontiguousarray(view), view=view, tag="odd")
    # the aligned form with strides beyond the rows: multiples of 4 throughout
    n, h, w = 4, 13, 1028
    store = np.random.default_rng(10).integers(0, 256, size=n * (h + 1) * 1040, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(store, shape=(n, h, w), strides=((h + 1) * 1040, 1040, 1))
    _check_minima(pkg, torch, eng, np.ascontiguousarray(view), view=view, tag="aligned-strided")


def test_minima_capacity(pkg, torch, eng):
    ffi = pkg._ffi
    cube = cc.random_cube(5, 13, 33, 4)
    want, want_offs = cc.per_slice_minima(cube, ol.find_local_minima)
    rc, got, offs, total, intact = _device_minima(pkg, torch, eng, cube, cap=len(want) - 1)
    assert rc == ffi.WS_ERR_CAPACITY and total == len(want) and intact
    assert (got == want[:-1]).all() and (offs == want_offs).all()
    rc, _, offs, total, intact = _device_minima(pkg, torch, eng, cube, cap=0, null_list=True)
    assert rc == ffi.WS_ERR_CAPACITY and total == len(want) and intact and (offs == want_offs).all()
    rc, _, offs, total, _ = _device_minima(pkg, torch, eng, cc.seedless_cube()[:1], cap=0, null_list=True)      # nothing to write: no error
    assert rc == 0 and total == 0 and (offs == 0).all()


def test_minima_runs_under_the_batch_pixel_limit(pkg, torch, eng):
    cube = cc.random_cube(5, 9, 33, 8)
    want, want_offs = cc.per_slice_minima(cube, ol.find_local_minima)
    eng.ctx.set_batch_pixel_limit(2 * 9 * 33 + 5)      # runs of 2, 2 and 1 slices
    try:
        rc, got, offs, total, intact = _device_minima(pkg, torch, eng, cube)
        assert rc == 0 and intact and total == len(want) and (offs == want_offs).all() and (got[:total] == want).all()
        rc, got, offs, total, intact = _device_minima(pkg, torch, eng, cube, cap=int(want_offs[2]) + 1)      # the cut falls into the second run
        assert rc == pkg._ffi.WS_ERR_CAPACITY and intact and total == len(want) and (offs == want_offs).all()
        assert (got == want[:int(want_offs[2]) + 1]).all()
    finally:
        eng.ctx.set_batch_pixel_limit(0)


def test_minima_of_many_slices(pkg, torch, eng):
    n = 65537
    base = cc.random_cube(64, 8, 16, 21)
    cube = base[np.arange(n) % 61]      # (the period is not one of the strips': 61 slices x 8 rows)
    cube = np.ascontiguousarray(cube)
    cube[n - 1] = base[63]
    want61, offs61 = cc.per_slice_minima(base, ol.find_local_minima)
    counts = np.diff(offs61).astype(np.int64)
    per = counts[np.arange(n) % 61]
    per[n - 1] = counts[63]
    want_offs = np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)
    rc, got, offs, total, intact = _device_minima(pkg, torch, eng, cube)
    assert rc == 0 and intact and total == int(want_offs[-1]) and (offs == want_offs).all()
    for k in (0, 1, 60, 61, 8191, 8192, 32768, 65535, 65536):
        src = 63 if k == n - 1 else k % 61
        assert (got[int(offs[k]):int(offs[k + 1])] == want61[int(offs61[src]):int(offs61[src + 1])]).all(), k
    # every slice: the lists repeat with the slices
    first = got[:int(want_offs[61])]
    reps = (n - 1) // 61
    assert (got[:reps * len(first)].reshape(reps, -1) == first.reshape(1, -1)).all()


def test_host_minima_shim(pkg, ws):
    cube = cc.border_maxima_cube()
    want, want_offs = cc.per_slice_minima(cube, ol.find_local_minima)
    seeds, offs = ws.find_local_minima_cube(cube)
    assert seeds.dtype == np.uint64 and (seeds == want).all() and (offs == want_offs).all()
    seeds, offs = ws.find_local_minima_cube(np.zeros((3, 2, 9), np.uint8))
    assert seeds.shape == (0, 2) and (offs == 0).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def test_float_channel_last_cube_to_cut_catalogue(pkg, torch, eng, ws):
    """An f32 cube with the slice index last goes in; pre_processor_batch, find_local_minima_batch and merge_tree_cut_catalogue_batch
    give what the host shim gives with seeds=None on the cube pre-processed slice by slice by the oracle."""
    n, h, w = 4, 16, 32
    rng = np.random.default_rng(17)
    field = rng.normal(size=(h, w, n)).astype(np.float32) * (1 + np.arange(n, dtype=np.float32))      # every slice its own range
    field[3, 5, :] = np.nan
    u8 = np.stack([ol.pre_processor(np.ascontiguousarray(field[:, :, k])) for k in range(n)])
    cuts = [pkg.api.Cut(), pkg.api.Cut(min_area=3, show_level=200, merge_level=120)]
    want = ws.merge_tree_cut_catalogue_cube(u8, None, cuts)
    cube = eng.pre_processor_batch(torch.from_numpy(field).to(eng.device), axis=2)
    assert (cube.cpu().numpy() == u8).all()
    seeds, offs = eng.find_local_minima_batch(cube)
    res = eng.merge_tree_cut_catalogue_batch(cube, seeds, offs, cuts)
    torch.cuda.synchronize()
    assert len(want) == n
    for k in range(n):
        planes, lakes, region, offsets, hidden, hidden_stats = res["slices"][k]
        w_planes, w_lakes, w_region, w_offsets, w_hidden, w_hidden_stats = want[k][:6]
        assert (planes.cpu().numpy().view(np.uint32) == w_planes).all(), k
        assert (lakes.cpu().numpy().astype(np.uint64).reshape(-1) == np.frombuffer(np.ascontiguousarray(w_lakes).tobytes(), np.uint64)).all(), k
        assert region.cpu().numpy().tobytes() == np.ascontiguousarray(w_region).tobytes(), k
        assert (np.asarray(offsets) == np.asarray(w_offsets)).all() and (np.asarray(hidden) == np.asarray(w_hidden)).all(), k
        assert np.ascontiguousarray(hidden_stats).tobytes() == np.ascontiguousarray(w_hidden_stats).tobytes(), k
