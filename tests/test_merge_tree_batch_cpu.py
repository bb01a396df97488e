"""merge_tree of a cube of slices (ws_merge_tree_batch(_device)) without a GPU: the new symbols at the boundary and the argument
checks that come before any context exists.  Everything that needs a device is in tests/test_gpu_merge_tree_batch.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ws_merge_tree_batch_device", "ws_merge_tree_batch")


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


def test_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "ws_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "src", "hip_ffi.rs")).read()
    raw = ctypes.CDLL(pkg._ffi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in pkg._ffi.SIGNATURES
        assert getattr(raw, name) is not None
        assert re.search(r"\bpub fn " + name + r"\s*\(", rust), name
    assert pkg._ffi.lib().ws_abi_version() == pkg._ffi.WS_ABI_VERSION == 3


def test_mirror_header_and_rust_shim_name_the_method():
    assert "merge_tree_cube(" in open(os.path.join(ROOT, "include", "ws_watershed.hpp")).read()
    assert "fn merge_tree_cube(" in open(os.path.join(ROOT, "rust", "src", "watershed_hip.rs")).read()


def test_null_context_is_bad_arg(pkg):
    L = pkg._ffi.lib()
    opt = pkg._ffi.Options()
    cube = np.zeros((2, 4, 4), dtype=np.uint8)
    seeds32 = np.zeros((2, 2), dtype=np.uint32)
    seeds64 = np.zeros((2, 2), dtype=np.uint64)
    offs = (ctypes.c_size_t * 3)(0, 1, 2)
    tree = np.full((4, 4), 7, dtype=np.uint32)
    total = ctypes.c_size_t(99)
    failed = ctypes.c_size_t(99)
    rc = L.ws_merge_tree_batch_device(None, cube.ctypes.data, 2, 4, 4, 4, 16, seeds32.ctypes.data, offs, ctypes.byref(opt),
                                      tree.ctypes.data, None, ctypes.byref(failed))
    assert rc == pkg._ffi.WS_ERR_BAD_ARG
    rc = L.ws_merge_tree_batch(None, cube.ctypes.data, 2, 4, 4, 4, 16, seeds64.ctypes.data, offs, ctypes.byref(opt),
                               tree.ctypes.data, 4, ctypes.byref(total), None, None, ctypes.byref(failed))
    assert rc == pkg._ffi.WS_ERR_BAD_ARG
    assert (tree == 7).all() and total.value == 99


def test_wrapper_refuses_bad_cubes_before_any_context(pkg):
    ws = pkg.TransformBuilder.new().build_merging()
    with pytest.raises(ValueError):
        ws.merge_tree_cube(np.zeros((8, 8), dtype=np.uint8))                       # not 3-D
    with pytest.raises(ValueError):
        ws.merge_tree_cube(np.zeros((2, 3, 8, 8), dtype=np.uint8))
    with pytest.raises(ValueError):
        ws.merge_tree_cube(np.zeros((3, 8, 8), dtype=np.uint8), seeds=[[(1, 1)], [(2, 2)]])      # two lists, three slices
    with pytest.raises(ValueError):
        ws.merge_tree_cube(np.zeros((2, 8, 8), dtype=np.float32))                  # not u8
    with pytest.raises(ValueError):
        ws.merge_tree_cube(np.zeros((2, 8, 8), dtype=np.int32), seeds=[[(1, 1)], [(2, 2)]])


def test_segmenting_wrapper_has_no_tree_cube(pkg):
    assert hasattr(pkg.MergingWatershed, "merge_tree_cube") and not hasattr(pkg.SegmentingWatershed, "merge_tree_cube")
