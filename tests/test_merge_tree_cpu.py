"""merge_tree without a GPU: the new symbols at the boundary, the argument checks that come before any device work, and the
numpy derivation of the tree from the CPU oracle's planes (tests/merge_tree_ref.py) against the invariants the definition promises.
A context cannot be created without a device, and every check but the null context needs one to report through: the null-pointer,
option and in-flight refusals are in tests/test_gpu_merge_tree.py (test_argument_checks_come_before_device_work)."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import merge_tree_ref as mt
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ws_merge_tree_device", "ws_merge_tree")


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


def test_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "ws_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(pkg._ffi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in pkg._ffi.SIGNATURES
        assert getattr(raw, name) is not None
    assert "typedef struct ws_tree_node" in code and "#define WS_TREE_ALIVE 0xFFFFFFFFu" in code
    assert pkg._ffi.lib().ws_abi_version() == pkg._ffi.WS_ABI_VERSION == 3
    assert ctypes.sizeof(pkg._ffi.TreeNode) == 16
    assert [f for f, _ in pkg._ffi.TreeNode._fields_] == ["parent", "death_level", "area", "n_leaves"]
    assert pkg._ffi.WS_TREE_ALIVE == 0xFFFFFFFF == pkg.MergeTree.ALIVE


def test_null_context_is_bad_arg(pkg):
    L = pkg._ffi.lib()
    opt = pkg._ffi.Options()
    img = np.zeros((4, 4), dtype=np.uint8)
    seeds = np.zeros((1, 2), dtype=np.uint64)
    tree = np.zeros((2, 4), dtype=np.uint32)
    for name in NEW:
        rc = getattr(L, name)(None, img.ctypes.data, 4, 4, 4, seeds.ctypes.data, 1, ctypes.byref(opt), tree.ctypes.data, None)
        assert rc == pkg._ffi.WS_ERR_BAD_ARG, name


def test_mirror_header_and_rust_shim_name_the_method():
    assert "merge_tree" in open(os.path.join(ROOT, "include", "ws_watershed.hpp")).read()
    assert "merge_tree" in open(os.path.join(ROOT, "rust", "src", "watershed_hip.rs")).read()
    assert "ws_merge_tree" in open(os.path.join(ROOT, "rust", "src", "hip_ffi.rs")).read()


def test_segmenting_wrapper_has_no_tree(pkg):
    assert hasattr(pkg.MergingWatershed, "merge_tree") and not hasattr(pkg.SegmentingWatershed, "merge_tree")


@pytest.mark.parametrize("shape,seed,edge", [((50, 70), 2, False), ((96, 96), 3, True)])
def test_reference_tree_holds_the_invariants_on_random_fields(shape, seed, edge):
    img = cases.field(*shape, seed)
    seeds = ol.find_local_minima(img)
    parent, death, area, leaves, vals, ex = mt.expected_tree(img, seeds, edge=edge)
    mt.check_invariants(parent, death, area, leaves, vals, ex)
    alive = (death == mt.ALIVE) & ex
    ph, pw = img.shape[0] + (2 if edge else 0), img.shape[1] + (2 if edge else 0)
    assert int(area[alive].sum()) + int(area[0]) == ph * pw
    assert int(leaves[alive].sum()) == int(ex.sum())


def test_reference_tree_holds_the_invariants_on_adversarial_cases():
    for name, img, seeds in cases.adversarial_cases():
        seeds = cases.seeds_or_maxima(img, seeds)
        for edge in (False, True):
            parent, death, area, leaves, vals, ex = mt.expected_tree(img, seeds, edge=edge)
            mt.check_invariants(parent, death, area, leaves, vals, ex)
            assert parent.size == len(seeds) + 1, (name, edge)


def test_roots_at_and_children_on_a_hand_made_tree(pkg):
    A = pkg.MergeTree.ALIVE
    #        0  1  2  3  4  5  6      colour 6 never was; 5 -> 3 at level 2, 3 -> 2 at 7, 4 -> 2 at 7, 2 -> 1 at 40
    parent = [0, 0, 1, 2, 2, 3, 0]
    death = [A, A, 40, 7, 7, 2, A]
    t = pkg.MergeTree(parent, death, [9, 50, 20, 6, 1, 2, 0], [0, 5, 4, 2, 1, 1, 0])
    assert t.roots_at(0).tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert t.roots_at(1).tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert t.roots_at(2).tolist() == [0, 1, 2, 3, 4, 3, 6]
    assert t.roots_at(6).tolist() == [0, 1, 2, 3, 4, 3, 6]
    assert t.roots_at(7).tolist() == [0, 1, 2, 2, 2, 2, 6]
    assert t.roots_at(39).tolist() == [0, 1, 2, 2, 2, 2, 6]
    assert t.roots_at(40).tolist() == [0, 1, 1, 1, 1, 1, 6]
    assert t.roots_at(254).tolist() == [0, 1, 1, 1, 1, 1, 6]
    assert t.roots_at(254).dtype == np.uint32 and t.roots_at(3)[0] == 0
    kids = t.children()
    assert {k: v.tolist() for k, v in kids.items()} == {1: [2], 2: [3, 4], 3: [5]}
    for L in (0, 2, 7, 40):
        assert (t.roots_at(L) == mt.roots_at(t.parent, t.death_level, L)).all()
