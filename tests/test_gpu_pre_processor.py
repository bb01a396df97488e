"""ws_pre_processor / ws_pre_processor_device (k_minmax, k_minmax_final, k_quantise of csrc/ws_preproc.hip) at their edges, -m gpu.

Every comparison is exact, on u8, against the C oracle (ol.pre_processor) cross-checked by the numpy restatement
(ol.pre_processor_numpy); nothing is compared with the engine itself.  The inputs come from tests/preproc_cases.py, whose claims
(which index holds which extreme, which block owns which partial, that the rounding set can tell a reordered quantiser from the
reference's) are checked on the CPU in tests/test_pre_processor.py.

  placed extrema     a lost lane, wave, block or partial of the reduction: one unique minimum and maximum at chosen indices
  beyond the caps    the trips a capped grid adds to both grid-stride loops; the 4096-partial walk of k_minmax_final
  rounding order     (v - min) / range, then * MAX: integer ramps on which any other order is wrong somewhere
  range overflow     max - min = +inf: WS_ERR_UNSUPPORTED where the reference panics (lib.rs:1164)
  device entry       unaligned windows of larger buffers, argument checks, interleaved with captured transforms on one context
"""
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import merge_tree_ref as mt
import oracle_lib as ol
import preproc_cases as pc

pytestmark = pytest.mark.gpu

GUARD = 0xA5


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def eng(pkg):
    import torch
    with torch.cuda.stream(torch.cuda.Stream(0)):      # a stream of its own: the transforms of the interleaving test are captured and replayed
        yield importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


@pytest.fixture(scope="module")
def ws(pkg):
    return pkg.TransformBuilder.default().build_segmenting()


def _want(arr, mx=254):
    a = ol.pre_processor(arr, mx)
    assert (a == ol.pre_processor_numpy(arr, mx)).all()      # the reference of every GPU result: two restatements that agree
    return a


def _bytes_to_dev(eng, arr, lead=0, tail=0):
    """The array's bytes on the device behind `lead` and before `tail` bytes of 0xFF (as f32 / f64: NaN)."""
    import torch
    raw = np.concatenate([np.full(lead, 0xFF, np.uint8), np.ascontiguousarray(arr).view(np.uint8).reshape(-1), np.full(tail, 0xFF, np.uint8)])
    return torch.from_numpy(raw).to(eng.device)


def _device_call(pkg, eng, arr, mx=254, in_lead=0, out_lead=0, out_tail=64):
    """ws_pre_processor_device on the array at byte offset in_lead of a larger buffer, into the window at byte offset out_lead of
    a guard-filled buffer.  Returns (status, the window, whether every byte around the window still is the guard)."""
    import torch
    arr = np.ascontiguousarray(arr).reshape(-1)
    t_in = _bytes_to_dev(eng, arr, in_lead, 16)
    t_out = torch.full((out_lead + arr.size + out_tail,), GUARD, dtype=torch.uint8, device=eng.device)
    rc = pkg._ffi.lib().ws_pre_processor_device(eng.ctx.handle, t_in.data_ptr() + in_lead, pkg._ffi.WS_DTYPES[arr.dtype.name], arr.size,
                                                mx, t_out.data_ptr() + out_lead)
    torch.cuda.synchronize()
    got = t_out.cpu().numpy()
    around = np.concatenate([got[:out_lead], got[out_lead + arr.size:]])
    return rc, got[out_lead:out_lead + arr.size], bool((around == GUARD).all())


# ---- 1. range overflow ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,arr", pc.overflow_arrays(), ids=[c[0] for c in pc.overflow_arrays()])
def test_range_overflow_is_refused_by_both_entry_points(pkg, eng, ws, name, arr):
    ffi = pkg._ffi
    with pytest.raises(ol.ReferencePanics):
        ol.pre_processor(arr)
    near = np.array(pc.NEAR_MISS)
    for mx in (254, 1):
        # host form, through the Python API: raises as for every other negative status
        with pytest.raises(pkg.api.WatershedError, match="lib.rs:1164") as e:
            ws.pre_processor_with_max(arr, mx)
        assert e.value.status == ffi.WS_ERR_UNSUPPORTED
        # ... and raw
        out = np.full(arr.size, GUARD, dtype=np.uint8)
        ctx = ws._ctx()
        assert ffi.lib().ws_pre_processor(ctx.handle, arr.ctypes.data, ffi.WS_DTYPES["float64"], arr.size, mx, out.ctypes.data) == ffi.WS_ERR_UNSUPPORTED
        assert b"lib.rs:1164" in ffi.lib().ws_last_error(ctx.handle)
        # the next call on the same context works
        assert (ws.pre_processor_with_max(near, mx) == _want(near, mx)).all()
        # device form (the contents of its output are unspecified after the error; the bytes around it are not)
        rc, _, intact = _device_call(pkg, eng, arr, mx, in_lead=8, out_lead=1)
        assert rc == ffi.WS_ERR_UNSUPPORTED and intact
        assert b"lib.rs:1164" in ffi.lib().ws_last_error(eng.ctx.handle)
        rc, got, intact = _device_call(pkg, eng, near, mx, in_lead=8, out_lead=1)
        assert rc == ffi.WS_OK and intact and (got == _want(near, mx)).all()
    # the same values as f32 are +-inf: filtered out, no overflow
    with np.errstate(over="ignore"):
        as32 = arr.astype(np.float32)
    assert (ws.pre_processor(as32) == _want(as32)).all()


# ---- 2. placed extrema ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", pc.SIGNED + pc.UNSIGNED)
@pytest.mark.parametrize("n", pc.PLACED_N)
def test_placed_extrema(ws, n, dtype):
    """One unique minimum and one unique maximum in a constant array, at every index of the set in both roles: a lane, wave,
    block or partial that the reduction drops changes (almost) every output byte."""
    todo = pc.placed_cases(n, dtype)
    assert todo
    for tag, a in todo:
        got = ws.pre_processor(a)
        assert (got == _want(a)).all(), (n, dtype, tag)
    tag, a = todo[len(todo) // 2]
    assert (ws.pre_processor_with_max(a, 1) == _want(a, 1)).all(), (n, dtype, tag)


def test_placed_extrema_variants(ws):
    for tag, a in pc.variant_cases():
        for mx in (254, 3):
            assert (ws.pre_processor_with_max(a, mx) == _want(a, mx)).all(), (tag, mx)


# ---- 3. beyond the block caps --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,make", pc.beyond_cap_cases(), ids=[c[0] for c in pc.beyond_cap_cases()])
def test_beyond_the_block_caps(pkg, eng, tag, make):
    """n above 4096 * 2048 (k_minmax) and 16384 * 1024 (k_quantise): the grids are capped and every thread takes more trips; the
    extremes sit where only the added trips reach.  The output buffer is pre-filled: an element that no trip writes keeps the
    guard, and nothing is written behind the last element."""
    a = make()
    want = _want(a)
    assert not (want == GUARD).any()
    rc, got, intact = _device_call(pkg, eng, a, out_tail=4096)
    assert rc == pkg._ffi.WS_OK and intact
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (tag, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("blocks", [4095, 4096])
def test_every_partial_of_a_full_grid_counts(pkg, eng, blocks):
    """Exactly 4095 and exactly 4096 (the cap) k_minmax blocks, every block with extremes of its own: the global maximum is block
    300's partial and the global minimum the last block's, which k_minmax_final reaches in the last step of its walk."""
    a = pc.per_block_extremes(blocks)
    want = _want(a)
    rc, got, intact = _device_call(pkg, eng, a, out_tail=4096)
    assert rc == pkg._ffi.WS_OK and intact
    assert (got == want).all()
    # moved around: the global extremes in the first / last partial of the walk's last thread
    b = a.copy()
    b[(blocks - 1) * 256 + 5] = 30000                      # block blocks - 1, first trip
    b[255 * 256 + 9] = -30000                              # block 255
    rc, got, intact = _device_call(pkg, eng, b, out_tail=4096)
    assert rc == pkg._ffi.WS_OK and intact and (got == _want(b)).all()


# ---- 4. rounding order and value edges -----------------------------------------------------------------------------------------

def test_rounding_order_set_is_bit_exact(ws):
    """Integer ramps 0..R and -(R // 2)..R - R // 2 under every MAX of the set: a quantiser that multiplies before it divides, or
    by the reciprocal of the range, is wrong on some of them (counted in tests/test_pre_processor.py)."""
    mul_first, recip = pc.reordered_counts()
    assert mul_first > 0 and recip > 0
    for tag, a in pc.rounding_cases():
        for mx in pc.ROUNDING_MAX:
            got = ws.pre_processor_with_max(a, mx)
            want = _want(a, mx)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (tag, mx, bad[:8], got[bad[:8]], want[bad[:8]])


def test_value_edges(pkg, eng, ws):
    for tag, a in pc.value_edge_cases():
        for mx in (254, 127, 1):
            assert (ws.pre_processor_with_max(a, mx) == _want(a, mx)).all(), (tag, mx)
        rc, got, intact = _device_call(pkg, eng, a, out_lead=3)
        assert rc == pkg._ffi.WS_OK and intact and (got == _want(a)).all(), tag


# ---- 5. the device entry point -------------------------------------------------------------------------------------------------

def _six_dtypes(n, seed):
    rng = np.random.default_rng(seed)
    f64 = rng.normal(0, 50, n)
    if n >= 4:
        f64[[0, n // 2, n - 1, 1]] = [np.nan, np.inf, -np.inf, 0.0]
    f32 = f64.astype(np.float32)
    return [f64, f32, rng.integers(-10 ** 6, 10 ** 6, n, dtype=np.int32), rng.integers(0, 65536, n, dtype=np.uint16),
            rng.integers(-32768, 32768, n, dtype=np.int16), rng.integers(0, 256, n, dtype=np.uint8)]


@pytest.mark.parametrize("n", [1, 5, 1023, 2049, 70001])
def test_device_entry_on_unaligned_windows(pkg, eng, n):
    """Input at element-aligned offsets that are no multiple of 16 bytes, output at odd byte offsets, n no multiple of 4."""
    assert n % 4 != 0
    for a in _six_dtypes(n, n):
        item = a.dtype.itemsize
        for elems, out_lead in ((1, 1), (3, 3)):
            in_lead = elems * item if (elems * item) % 16 else (elems + 1) * item
            assert in_lead % item == 0 and in_lead % 16 != 0
            for mx in (254, 100):
                rc, got, intact = _device_call(pkg, eng, a, mx, in_lead=in_lead, out_lead=out_lead)
                assert rc == pkg._ffi.WS_OK, (a.dtype, n)
                assert intact, (a.dtype, n, "bytes around the output window changed")
                assert (got == _want(a, mx)).all(), (a.dtype, n, in_lead, out_lead, mx)


def test_device_entry_argument_checks(pkg, eng):
    import torch
    ffi = pkg._ffi
    L, h = ffi.lib(), eng.ctx.handle
    f64 = ffi.WS_DTYPES["float64"]
    t_in = _bytes_to_dev(eng, np.array([1.0, -2.0, 3.0]))
    t_out = torch.full((16,), GUARD, dtype=torch.uint8, device=eng.device)

    def untouched():
        torch.cuda.synchronize()
        return bool((t_out == GUARD).all())

    assert L.ws_pre_processor_device(h, None, f64, 3, 254, t_out.data_ptr()) == ffi.WS_ERR_BAD_ARG
    assert L.ws_pre_processor_device(h, t_in.data_ptr(), f64, 3, 254, None) == ffi.WS_ERR_BAD_ARG
    assert L.ws_pre_processor_device(h, None, f64, 0, 254, None) == ffi.WS_OK              # nothing to do, nothing written
    assert L.ws_pre_processor_device(h, t_in.data_ptr(), f64, 0, 254, t_out.data_ptr()) == ffi.WS_OK
    for bad_dtype in (-1, 6, 99):
        assert L.ws_pre_processor_device(h, t_in.data_ptr(), bad_dtype, 3, 254, t_out.data_ptr()) == ffi.WS_ERR_BAD_ARG
    assert L.ws_pre_processor_device(h, t_in.data_ptr(), f64, 3, 0, t_out.data_ptr()) == ffi.WS_ERR_MAX_TOO_LOW
    assert L.ws_pre_processor_device(h, t_in.data_ptr(), f64, 3, 255, t_out.data_ptr()) == ffi.WS_ERR_MAX_TOO_HIGH
    assert untouched()
    # the host form checks the same
    x = np.array([1.0, -2.0, 3.0])
    o = np.full(3, GUARD, dtype=np.uint8)
    assert L.ws_pre_processor(h, None, f64, 3, 254, o.ctypes.data) == ffi.WS_ERR_BAD_ARG
    assert L.ws_pre_processor(h, x.ctypes.data, f64, 3, 254, None) == ffi.WS_ERR_BAD_ARG
    assert L.ws_pre_processor(h, None, f64, 0, 254, None) == ffi.WS_OK
    assert L.ws_pre_processor(h, x.ctypes.data, 6, 3, 254, o.ctypes.data) == ffi.WS_ERR_BAD_ARG
    assert L.ws_pre_processor(h, x.ctypes.data, f64, 3, 0, o.ctypes.data) == ffi.WS_ERR_MAX_TOO_LOW
    assert L.ws_pre_processor(h, x.ctypes.data, f64, 3, 255, o.ctypes.data) == ffi.WS_ERR_MAX_TOO_HIGH
    assert (o == GUARD).all()
    # a context that holds a begun transform takes no other work
    img = cases.field(96, 128, 5)
    seeds = ol.find_local_minima(img)
    d_img = torch.from_numpy(img).to(eng.device)
    d_seeds = torch.from_numpy(seeds.astype(np.int64).astype(np.int32)).to(eng.device)
    labels = torch.zeros((96, 128), dtype=torch.int32, device=eng.device)
    eng.segment_begin(d_img, d_seeds, labels)
    try:
        assert L.ws_pre_processor_device(h, t_in.data_ptr(), f64, 3, 254, t_out.data_ptr()) == ffi.WS_ERR_BAD_ARG
        assert L.ws_pre_processor(h, x.ctypes.data, f64, 3, 254, o.ctypes.data) == ffi.WS_ERR_BAD_ARG
    finally:
        eng.segment_end()
    assert untouched() and (o == GUARD).all()
    assert (labels.cpu().numpy().view(np.uint32) == ol.segment(img, seeds)).all()
    # ... and takes it again afterwards
    assert L.ws_pre_processor_device(h, t_in.data_ptr(), f64, 3, 254, t_out.data_ptr()) == ffi.WS_OK
    torch.cuda.synchronize()
    assert (t_out.cpu().numpy()[:3] == _want(x)).all() and bool((t_out[3:] == GUARD).all())


def test_pre_processor_between_replayed_transforms_on_one_context(pkg):
    """The pre-processor shares the context's workspaces (counts, aux, img) with the transforms, whose captured graphs hold
    pointers into the context's buffers and must notice a reallocation (buffer_generation)."""
    import torch
    dev = importlib.import_module("rustronomy_watershed_amd.device")
    ffi = pkg._ffi
    with torch.cuda.stream(torch.cuda.Stream(0)):
        e = dev.DeviceEngine(0)                              # a fresh context: its workspaces are as small as the transforms made them
        img = cases.field(256, 320, 21)
        seeds = ol.find_local_minima(img)
        want_seg = ol.segment(img, seeds)
        want_tree = np.stack(mt.expected_tree(img, seeds)[:4], axis=1)
        d_img = torch.from_numpy(img).to(e.device)
        d_seeds = torch.from_numpy(seeds.astype(np.int64).astype(np.int32)).to(e.device)
        labels = torch.empty(img.shape, dtype=torch.int32, device=e.device)
        tree = torch.empty((len(seeds) + 1, 4), dtype=torch.int32, device=e.device)

        def segment():
            labels.zero_()
            e.segment(d_img, d_seeds, out=labels)
            torch.cuda.synchronize()
            assert (labels.cpu().numpy().view(np.uint32) == want_seg).all()
            return e.stats()["graph_launches"]

        def merge_tree():
            tree.zero_()
            e.merge_tree(d_img, d_seeds, out=tree)
            torch.cuda.synchronize()
            assert (tree.cpu().numpy().view(np.uint32) == want_tree).all()

        # the same transform again and again: captured once the context's workspaces have stopped growing (the second to the
        # fourth run), replayed as ONE graph launch from then on
        launches = [segment() for _ in range(5)]
        assert launches[-2:] == [1, 1], launches
        n = 1 << 22
        rng = np.random.default_rng(5)
        x = rng.normal(0, 1, n)
        x[[7, n - 3]] = [-9.0, 11.0]
        want_x = _want(x)
        d_x = torch.from_numpy(x).to(e.device)
        d_q = torch.full((n + 64,), GUARD, dtype=torch.uint8, device=e.device)
        assert ffi.lib().ws_pre_processor_device(e.ctx.handle, d_x.data_ptr(), ffi.WS_DTYPES["float64"], n, 254, d_q.data_ptr()) == ffi.WS_OK
        torch.cuda.synchronize()
        got = d_q.cpu().numpy()
        assert (got[:n] == want_x).all() and (got[n:] == GUARD).all()
        segment()
        host = np.empty(n, dtype=np.uint8)                   # the host form stages 32 MB + 4 MB in the context's aux and img buffers
        assert ffi.lib().ws_pre_processor(e.ctx.handle, x.ctypes.data, ffi.WS_DTYPES["float64"], n, 254, host.ctypes.data) == ffi.WS_OK
        assert (host == want_x).all()
        merge_tree()
        merge_tree()
        segment()
        y = x[: 4099].astype(np.float32)
        got = np.empty(y.size, dtype=np.uint8)
        assert ffi.lib().ws_pre_processor(e.ctx.handle, y.ctypes.data, ffi.WS_DTYPES["float32"], y.size, 254, got.ctypes.data) == ffi.WS_OK
        assert (got == _want(y)).all()
        segment()
