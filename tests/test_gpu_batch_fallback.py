"""The cube drivers' shared walk (csrc/ws_batch.hip, run_batch) where it leaves the stack: a late group that mispredicts after
earlier groups have written their output, a middle group without a seed, and an error that the slice-by-slice loop has to name.
Every product of the walk -- segment_batch, merge_batch, transform_to_list_batch segmenting and merging, transform_history_batch
merging -- against the same product computed slice by slice with the single-field call on a second context, bit for bit (lake
records per level as sets: their order within a level is not defined).

The cube: 7 slices of 32 x 64 with set_batch_pixel_limit(2 * 32 * 64), so the groups are 2 + 2 + 2 + 1."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import oracle_lib as ol

pytestmark = pytest.mark.gpu

S, H, W, LEVELS = 7, 32, 64, 255
HISTORY_LEVELS = [0, 100, 254]
PRODUCTS = ["segment", "merge", "lists_seg", "lists_mer", "history"]


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def cube():
    """Slices and sorted seed lists as test_gpu_parity.py's _batch_case builds them: the local minima of each slice plus seeds on its
    first / last row and in a corner.  Checked here with the oracle: every slice has a local minimum."""
    himgs, hseeds = [], []
    for k in range(S):
        a = cases.field(H, W, 900 + k) if k % 2 == 0 else cases.smooth_field(H, W, 900 + k)
        minima = ol.find_local_minima(a).astype(np.int64).reshape(-1, 2)
        assert len(minima) >= 1, k
        extra = np.array([[0, 0], [0, W // 2], [H - 1, 1], [H - 1, W - 1]], dtype=np.int64)
        himgs.append(a)
        hseeds.append(np.unique(np.concatenate([minima, extra]), axis=0))      # sorted row-major
    return np.stack(himgs), hseeds


def _engines(pkg):
    dev = importlib.import_module("rustronomy_watershed_amd.device")
    eng, ref = dev.DeviceEngine(0), dev.DeviceEngine(0)
    eng.ctx.set_batch_pixel_limit(2 * H * W)
    return eng, ref


def _to_device(torch, eng, himgs, lists):
    flat = np.concatenate(lists, axis=0).astype(np.int32).reshape(-1, 2)
    offs = [0] + [int(x) for x in np.cumsum([len(l) for l in lists])]
    seeds = [torch.from_numpy(np.ascontiguousarray(l.astype(np.int32).reshape(-1, 2))).to(eng.device) for l in lists]
    return torch.from_numpy(himgs).to(eng.device).contiguous(), torch.from_numpy(flat).to(eng.device).contiguous(), offs, seeds


def _level_keys(torch, lakes, offsets, k):
    """Slice k's records as one sorted key tensor (level, colour, area): equal keys = equal record sets at every level"""
    lo, hi = int(offsets[k * LEVELS]), int(offsets[(k + 1) * LEVELS])
    counts = torch.from_numpy(np.diff(offsets[k * LEVELS:(k + 1) * LEVELS + 1].astype(np.int64))).to(lakes.device)
    lvl = torch.repeat_interleave(torch.arange(LEVELS, device=lakes.device, dtype=torch.int64), counts)
    r = lakes[lo:hi]
    return torch.sort((lvl << 56) | (r[:, 0] << 28) | r[:, 1]).values


def _batch(pkg, torch, eng, product, d_cube, d_seeds, offs, cap=None):
    """The batch call through the C ABI: (status, failed_slice, result)"""
    L, hnd = pkg._ffi.lib(), eng.ctx.handle
    opt = eng.options(254, False)
    c_offs = (ctypes.c_size_t * (S + 1))(*offs)
    failed = ctypes.c_size_t(99)
    args = (d_cube.data_ptr(), S, H, W, W, H * W, d_seeds.data_ptr(), c_offs, ctypes.byref(opt))
    if product in ("segment", "merge"):
        out = torch.full((S, H, W), -1, dtype=torch.int32, device=eng.device)
        fn = L.ws_segment_batch_device if product == "segment" else L.ws_merge_batch_device
        return fn(hnd, *args, out.data_ptr(), ctypes.byref(failed)), failed.value, out
    if product == "history":
        lv = np.array(HISTORY_LEVELS, dtype=np.uint8)
        out = torch.full((S, len(lv), H, W), -1, dtype=torch.int32, device=eng.device)
        rc = L.ws_transform_history_batch_device(hnd, 1, *args, lv.ctypes.data, lv.size, out.data_ptr(), H * W, ctypes.byref(failed))
        return rc, failed.value, out
    if cap is None:
        cap = LEVELS * (offs[-1] + S)
    lakes = torch.zeros((max(cap, 1), 2), dtype=torch.int64, device=eng.device)
    offsets, unc, n = np.zeros(S * LEVELS + 1, dtype=np.uint64), np.zeros(S * LEVELS, dtype=np.uint64), ctypes.c_size_t(0)
    rc = L.ws_transform_to_list_batch_device(hnd, int(product == "lists_mer"), *args, lakes.data_ptr(), cap, ctypes.byref(n), offsets.ctypes.data,
                                             unc.ctypes.data, ctypes.byref(failed))
    return rc, failed.value, (n.value, offsets, unc, lakes)


def _single(ref, product, img, seeds):
    """The single-field call of one slice on the reference context"""
    if product == "segment":
        return ref.segment(img, seeds)
    if product == "merge":
        return ref.merge(img, seeds)
    if product == "history":
        return ref.transform_history(img, seeds, levels=HISTORY_LEVELS, merging=True)
    return ref.transform_to_list(img, seeds, merging=product == "lists_mer")


def _status(pkg, fn):
    try:
        fn()
    except pkg.SeedOutOfBounds:
        return pkg._ffi.WS_ERR_SEED_OOB
    except pkg.WatershedError as e:
        return e.status
    return pkg._ffi.WS_OK


def _assert_equal(torch, product, got, want, tag):
    if product in ("segment", "merge", "history"):
        for k in range(S):
            assert torch.equal(got[k], want[k]), (tag, product, k)
        return
    n, offsets, unc, lakes = got
    assert n == sum(len(w[0]) for w in want) and offsets[-1] == n, (tag, product)
    for k in range(S):
        one, off1, unc1 = want[k]
        assert (np.diff(offsets[k * LEVELS:(k + 1) * LEVELS + 1].astype(np.int64)) == np.diff(off1.astype(np.int64))).all(), (tag, product, k)
        assert (unc[k * LEVELS:(k + 1) * LEVELS] == unc1).all(), (tag, product, k)
        assert torch.equal(_level_keys(torch, lakes, offsets, k), _level_keys(torch, one, off1, 0)), (tag, product, k)


def _has_arrival(pkg, eng):
    p, hh, ww = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
    return pkg._ffi.lib().ws_last_arrival_device(eng.ctx.handle, ctypes.byref(p), ctypes.byref(hh), ctypes.byref(ww)) == pkg._ffi.WS_OK


def test_late_group_mispredicts(pkg, torch, cube):
    """Slice 5's list is shuffled: the third group mispredicts after two groups have written their output, and the loop redoes the
    batch.  With the list sorted again the same context takes the stack again.  Lists one record short: counted exactly."""
    himgs, sorted_lists = cube
    shuffled = [l.copy() for l in sorted_lists]
    shuffled[5] = shuffled[5][np.random.default_rng(5).permutation(len(shuffled[5]))]
    key = shuffled[5][:, 0] * W + shuffled[5][:, 1]
    assert (np.diff(key) < 0).any()      # really unsorted
    eng, ref = _engines(pkg)
    for product in PRODUCTS:
        for tag, lists in (("shuffled", shuffled), ("sorted", sorted_lists)):
            d_cube, d_seeds, offs, seeds = _to_device(torch, eng, himgs, lists)
            want = [_single(ref, product, d_cube[k], seeds[k]) for k in range(S)]
            rc, failed, got = _batch(pkg, torch, eng, product, d_cube, d_seeds, offs)
            assert rc == pkg._ffi.WS_OK and failed == 0, (tag, product, rc, failed)
            _assert_equal(torch, product, got, want, tag)
            if product == "segment":      # the loop leaves the last slice's stamps on the context, a stack leaves none: the stack was taken again
                assert _has_arrival(pkg, eng) == (tag == "shuffled"), tag
            if product.startswith("lists") and tag == "shuffled":
                rc, failed, short = _batch(pkg, torch, eng, product, d_cube, d_seeds, offs, cap=got[0] - 1)
                assert rc == pkg._ffi.WS_ERR_CAPACITY and short[0] == got[0], (product, rc, short[0], got[0])


def test_middle_group_has_no_seed(pkg, torch, cube):
    """Slices 2 and 3, the second group, have no seed: the loop takes the batch before anything is flooded"""
    himgs, lists = cube
    lists = [l[:0] if k in (2, 3) else l for k, l in enumerate(lists)]
    eng, ref = _engines(pkg)
    d_cube, d_seeds, offs, seeds = _to_device(torch, eng, himgs, lists)
    for product in ("segment", "merge"):
        want = [_single(ref, product, d_cube[k], seeds[k]) for k in range(S)]
        rc, failed, got = _batch(pkg, torch, eng, product, d_cube, d_seeds, offs)
        assert rc == pkg._ffi.WS_OK and failed == 0, (product, rc, failed)
        _assert_equal(torch, product, got, want, "empty group")
        assert int(got[2:4].abs().sum()) == 0 and int((got[1] != 0).sum()) > 0, product


def test_error_in_the_loop_is_named(pkg, torch, cube):
    """Slice 4 has a seed below its last row: every product reports the single-field call's status for that slice and names it;
    the context is usable afterwards"""
    himgs, good = cube
    bad = [np.concatenate([l, [[H, 5]]]) if k == 4 else l for k, l in enumerate(good)]
    eng, ref = _engines(pkg)
    d_cube, d_bad, bad_offs, bad_seeds = _to_device(torch, eng, himgs, bad)
    _, d_good, good_offs, good_seeds = _to_device(torch, eng, himgs, good)
    for product in PRODUCTS:
        want_rc = _status(pkg, lambda: _single(ref, product, d_cube[4], bad_seeds[4]))
        assert want_rc != pkg._ffi.WS_OK, product
        rc, failed, _ = _batch(pkg, torch, eng, product, d_cube, d_bad, bad_offs)
        assert rc == want_rc and failed == 4, (product, rc, want_rc, failed)
        want = [_single(ref, product, d_cube[k], good_seeds[k]) for k in range(S)]
        rc, failed, got = _batch(pkg, torch, eng, product, d_cube, d_good, good_offs)
        assert rc == pkg._ffi.WS_OK and failed == 0, (product, rc, failed)
        _assert_equal(torch, product, got, want, "after the error")
