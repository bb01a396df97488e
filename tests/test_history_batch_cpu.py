"""CPU-side checks of transform_history for a cube of slices (ws_transform_history_batch(_device)): exported and declared in
every mirror, the checks the C entry points make before any device work, and the Python wrappers' refusals before any
context is made."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge

NEW = ("ws_transform_history_batch_device", "ws_transform_history_batch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


def test_batch_history_symbols_exported_and_declared(pkg):
    raw = ctypes.CDLL(pkg._ffi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "ws_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "hip_ffi.rs")).read()
    for name in NEW:
        assert name in pkg._ffi.SIGNATURES
        assert getattr(raw, name) is not None
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
        assert re.search(rf"pub fn {name}\(", rust), name
    assert pkg._ffi.lib().ws_abi_version() == 3
    assert "transform_history_cube(" in open(os.path.join(ROOT, "include", "ws_watershed.hpp")).read()
    assert "fn transform_history_cube(" in open(os.path.join(ROOT, "rust", "src", "watershed_hip.rs")).read()


def test_null_context_is_refused(pkg):
    # no context can be made without a device: the checks that come before any device work answer WS_ERR_BAD_ARG
    L = pkg._ffi.lib()
    opt = pkg._ffi.Options()
    bad = pkg._ffi.WS_ERR_BAD_ARG
    levels = np.array([0, 3, 254], dtype=np.uint8)
    cube = np.zeros((2, 8, 8), dtype=np.uint8)
    seeds = np.array([[3, 3], [4, 4]], dtype=np.uint64)
    offs = (ctypes.c_size_t * 3)(0, 1, 2)
    out = np.zeros((2, 3, 8, 8), dtype=np.uint64)
    failed = ctypes.c_size_t(5)
    assert L.ws_transform_history_batch(None, 1, cube.ctypes.data, 2, 8, 8, 8, 64, seeds.ctypes.data, offs, ctypes.byref(opt),
                                        levels.ctypes.data, 3, out.ctypes.data, None, ctypes.byref(failed)) == bad
    assert L.ws_transform_history_batch_device(None, 0, None, 2, 8, 8, 8, 64, None, offs, ctypes.byref(opt), levels.ctypes.data, 3,
                                               None, 64, ctypes.byref(failed)) == bad


@pytest.mark.parametrize("build", ["build_segmenting", "build_merging"])
def test_python_wrapper_refuses_bad_cubes_and_levels_without_a_device(pkg, build):
    ws = getattr(pkg.TransformBuilder.default().set_max_water_lvl(100), build)()
    cube = np.zeros((3, 8, 8), np.uint8)
    seeds = [[(3, 3)], [(4, 4)], [(2, 5)]]
    with pytest.raises(ValueError):
        ws.transform_history_cube(np.zeros((8, 8), np.uint8), seeds[:1], [0])                # a plane, not a cube
    with pytest.raises(ValueError):
        ws.transform_history_cube(cube, seeds[:2], [0])                                    # two seed lists for three slices
    for levels in ([101], [-1], [0, 300], list(range(100)) * 3, [0.5]):
        with pytest.raises(ValueError):
            ws.transform_history_cube(cube, seeds, levels)
    with pytest.raises(ValueError):
        ws.transform_history_cube(cube, seeds, [0, 1], out=np.zeros((3, 2, 8, 7), np.uint64))
    got = ws.transform_history_cube(cube, seeds, [])                                      # nothing asked, nothing run
    assert len(got) == 3 and all(g == [] for g in got)


def test_device_wrapper_refuses_bad_arguments_without_a_device(pkg):
    import importlib
    import torch
    dev = importlib.import_module("rustronomy_watershed_amd.device")
    eng = object.__new__(dev.DeviceEngine)      # the refusals come before any device work: no context needed
    cube = torch.zeros((2, 8, 8), dtype=torch.uint8)
    seeds = torch.zeros((0, 2), dtype=torch.int32)
    with pytest.raises(ValueError):
        eng.transform_history_batch(cube[0], seeds, [0, 0], levels=[0])
    with pytest.raises(ValueError):
        eng.transform_history_batch(cube, seeds, [0, 0, 0, 0], levels=[0])
    for levels in ([255], [10, 61], [-3], list(range(60)) * 5):
        with pytest.raises(ValueError):
            eng.transform_history_batch(cube, seeds, [0, 0, 0], levels=levels, max_level=60)
