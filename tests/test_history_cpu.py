"""CPU-side checks of transform_history for chosen levels (ws_transform_history(_device)): exported and declared, the checks
the C entry points make before any device work, and the Python wrappers' refusals of bad level lists."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge

NEW = ("ws_transform_history_device", "ws_transform_history")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


def test_history_symbols_exported_and_declared(pkg):
    raw = ctypes.CDLL(pkg._ffi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "ws_hip.h")).read()
    for name in NEW:
        assert name in pkg._ffi.SIGNATURES
        assert getattr(raw, name) is not None
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
    assert pkg._ffi.lib().ws_abi_version() == 3
    assert "transform_history_levels(" in open(os.path.join(ROOT, "include", "ws_watershed.hpp")).read()


def test_null_context_is_refused(pkg):
    # no context can be made without a device: the checks that come before any device work answer WS_ERR_BAD_ARG
    L = pkg._ffi.lib()
    opt = pkg._ffi.Options()
    bad = pkg._ffi.WS_ERR_BAD_ARG
    levels = np.array([0, 3, 254], dtype=np.uint8)
    out = np.zeros((3, 8, 8), dtype=np.uint64)
    img = np.zeros((8, 8), dtype=np.uint8)
    seeds = np.array([[3, 3]], dtype=np.uint64)
    assert L.ws_transform_history(None, 1, img.ctypes.data, 8, 8, 8, seeds.ctypes.data, 1, ctypes.byref(opt), levels.ctypes.data, 3,
                                  out.ctypes.data) == bad
    assert L.ws_transform_history_device(None, 0, None, 8, 8, 8, None, 1, ctypes.byref(opt), levels.ctypes.data, 3, None, 64) == bad


@pytest.mark.parametrize("build", ["build_segmenting", "build_merging"])
def test_python_wrapper_refuses_bad_levels_without_a_device(pkg, build):
    ws = getattr(pkg.TransformBuilder.default().set_max_water_lvl(100), build)()
    img = np.zeros((8, 8), np.uint8)
    for levels in ([101], [-1], [0, 300], list(range(100)) * 3, [0.5]):
        with pytest.raises(ValueError):
            ws.transform_history_levels(img, [(3, 3)], levels)
    assert ws.transform_history_levels(img, [(3, 3)], []) == []      # nothing asked, nothing run


def test_device_wrapper_refuses_bad_levels_without_a_device(pkg):
    import importlib
    import torch
    dev = importlib.import_module("rustronomy_watershed_amd.device")
    eng = object.__new__(dev.DeviceEngine)      # the refusals come before any device work: no context needed
    img = torch.zeros((8, 8), dtype=torch.uint8)
    seeds = torch.zeros((0, 2), dtype=torch.int32)
    for levels in ([255], [10, 61], [-3], list(range(60)) * 5):
        with pytest.raises(ValueError):
            eng.transform_history(img, seeds, levels=levels, max_level=60)


def test_level_list_normalisation(pkg):
    api = pkg.api
    assert api._history_levels(None, 3).tolist() == [0, 1, 2, 3]
    got = api._history_levels([7, 0, 7, 254], 254)
    assert got.dtype == np.uint8 and got.tolist() == [7, 0, 7, 254]
    assert api._history_levels(np.array([], dtype=np.int64), 10).size == 0
