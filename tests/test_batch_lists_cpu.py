"""CPU-side checks of the batched transform_to_list / merging entry points (ws_transform_to_list_batch(_device),
ws_merge_batch_device): exported, argument checks that need no device, and the Python wrappers' refusals."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as ge

NEW = ("ws_transform_to_list_batch_device", "ws_transform_to_list_batch", "ws_merge_batch_device")


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


def _offsets(*v):
    return (ctypes.c_size_t * len(v))(*v)


def test_batch_symbols_exported(pkg):
    raw = ctypes.CDLL(pkg._ffi.LIB_PATH)
    for name in NEW:
        assert name in pkg._ffi.SIGNATURES
        assert getattr(raw, name) is not None
    assert pkg._ffi.lib().ws_abi_version() == 3


def _call_lists_device(pkg, ctx, offs, slice_stride=64 * 64):
    L = pkg._ffi.lib()
    opt = pkg._ffi.Options()
    levels = opt.max_water_level + 1
    n = ctypes.c_size_t(0)
    failed = ctypes.c_size_t(0)
    offsets = np.zeros(3 * levels + 1, dtype=np.uint64)
    unc = np.zeros(3 * levels, dtype=np.uint64)
    return L.ws_transform_to_list_batch_device(ctx, 1, None, 3, 64, 64, 64, slice_stride, None, offs, ctypes.byref(opt), None, 0,
                                               ctypes.byref(n), offsets.ctypes.data, unc.ctypes.data, ctypes.byref(failed))


def test_null_context_is_refused(pkg):
    L = pkg._ffi.lib()
    opt = pkg._ffi.Options()
    bad = pkg._ffi.WS_ERR_BAD_ARG
    assert _call_lists_device(pkg, None, _offsets(0, 1, 2, 3)) == bad
    n = ctypes.c_size_t(0)
    offsets = np.zeros(3 * 255 + 1, dtype=np.uint64)
    unc = np.zeros(3 * 255, dtype=np.uint64)
    cube = np.zeros((3, 8, 8), dtype=np.uint8)
    assert L.ws_transform_to_list_batch(None, 0, cube.ctypes.data, 3, 8, 8, 8, 64, None, None, ctypes.byref(opt), None, 0,
                                        ctypes.byref(n), offsets.ctypes.data, unc.ctypes.data, None, None) == bad
    assert L.ws_merge_batch_device(None, None, 3, 64, 64, 64, 64 * 64, None, _offsets(0, 1, 2, 3), ctypes.byref(opt), None, None) == bad


def test_decreasing_offsets_and_short_slice_stride_are_refused(pkg):
    # no context can be made without a device: the checks that come before any device work answer WS_ERR_BAD_ARG either way
    L = pkg._ffi.lib()
    opt = pkg._ffi.Options()
    bad = pkg._ffi.WS_ERR_BAD_ARG
    assert _call_lists_device(pkg, None, _offsets(0, 2, 1, 3)) == bad
    assert _call_lists_device(pkg, None, _offsets(0, 1, 2, 3), slice_stride=64 * 63) == bad
    assert L.ws_merge_batch_device(None, None, 3, 64, 64, 64, 64 * 64, None, _offsets(0, 2, 1, 3), ctypes.byref(opt), None, None) == bad
    assert L.ws_merge_batch_device(None, None, 3, 64, 64, 64, 100, None, _offsets(0, 1, 2, 3), ctypes.byref(opt), None, None) == bad


def test_python_wrappers_refuse_bad_cubes_without_a_device(pkg):
    for build in ("build_segmenting", "build_merging"):
        ws = getattr(pkg.TransformBuilder.default(), build)()
        with pytest.raises(ValueError):
            ws.transform_to_list_cube(np.zeros((8, 8), np.uint8))
        with pytest.raises(ValueError):
            ws.transform_to_list_cube(np.zeros((3, 8, 8), np.uint8), seeds=[[(1, 1)], [(2, 2)]])
    import importlib
    import torch
    dev = importlib.import_module("rustronomy_watershed_amd.device")
    eng = object.__new__(dev.DeviceEngine)      # the refusals come before any device work: no context needed
    seeds = torch.zeros((0, 2), dtype=torch.int32)
    with pytest.raises(ValueError):
        eng.transform_to_list_batch(torch.zeros((8, 8), dtype=torch.uint8), seeds, [0, 0])
    with pytest.raises(ValueError):
        eng.transform_to_list_batch(torch.zeros((3, 8, 8), dtype=torch.uint8), seeds, [0, 0, 0])
    with pytest.raises(ValueError):
        eng.merge_batch(torch.zeros((3, 8, 8), dtype=torch.uint8), seeds, [0, 0])
