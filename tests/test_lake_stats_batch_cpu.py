"""merge_tree_stats of a cube of slices (ws_merge_tree_stats_batch(_device)) without a GPU: the new symbols at the boundary, the
argument checks that come before any context exists, and -- with numpy and the CPU oracle alone -- the proof that the inputs of
tests/test_gpu_lake_stats_batch.py reach the regimes its tests name.  Everything that needs a device is in that file."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import lake_stats_batch_cases as bc
import lake_stats_ref as ls
import merge_tree_ref as mt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ws_merge_tree_stats_batch_device", "ws_merge_tree_stats_batch")


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


def test_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "ws_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "src", "hip_ffi.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    raw = ctypes.CDLL(pkg._ffi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in pkg._ffi.SIGNATURES
        assert getattr(raw, name) is not None
        assert re.search(r"\bpub fn " + name + r"\s*\(", rust), name
        assert re.search(r"\bfn\s+" + name + r"\s*\(", doc), name
    assert pkg._ffi.lib().ws_abi_version() == pkg._ffi.WS_ABI_VERSION == 3


def test_mirror_header_and_rust_shim_name_the_method(pkg):
    assert "merge_tree_stats_cube(" in open(os.path.join(ROOT, "include", "ws_watershed.hpp")).read()
    assert "fn merge_tree_stats_cube(" in open(os.path.join(ROOT, "rust", "src", "watershed_hip.rs")).read()
    device = open(os.path.join(ROOT, "rustronomy-watershed_amd", "device.py")).read()
    assert "def merge_tree_stats_batch(" in device
    assert "ws_merge_tree_stats_batch" in open(os.path.join(ROOT, "tools", "trace_lists_entrypoints.py")).read()


def test_null_context_is_bad_arg(pkg):
    L = pkg._ffi.lib()
    opt = pkg._ffi.Options()
    cube = np.zeros((2, 4, 4), dtype=np.uint8)
    wt = np.zeros((2, 4, 4), dtype=np.uint16)
    seeds32 = np.zeros((2, 2), dtype=np.uint32)
    seeds64 = np.zeros((2, 2), dtype=np.uint64)
    offs = (ctypes.c_size_t * 3)(0, 1, 2)
    tree = np.full((4, 4), 7, dtype=np.uint32)
    stats = np.full(4 * 9, 7, dtype=np.uint64)
    labels = np.full((2, 4, 4), 7, dtype=np.uint64)
    total = ctypes.c_size_t(99)
    failed = ctypes.c_size_t(99)
    U16 = pkg._ffi.WS_DTYPES["uint16"]
    rc = L.ws_merge_tree_stats_batch_device(None, cube.ctypes.data, 2, 4, 4, 4, 16, seeds32.ctypes.data, offs, ctypes.byref(opt),
                                            wt.ctypes.data, U16, 4, 16, tree.ctypes.data, stats.ctypes.data, None, ctypes.byref(failed))
    assert rc == pkg._ffi.WS_ERR_BAD_ARG
    rc = L.ws_merge_tree_stats_batch(None, cube.ctypes.data, 2, 4, 4, 4, 16, seeds64.ctypes.data, offs, ctypes.byref(opt), wt.ctypes.data, U16,
                                     4, 16, tree.ctypes.data, stats.ctypes.data, 4, ctypes.byref(total), labels.ctypes.data, None,
                                     ctypes.byref(failed))
    assert rc == pkg._ffi.WS_ERR_BAD_ARG
    assert (tree == 7).all() and (stats == 7).all() and (labels == 7).all() and total.value == 99


def test_wrapper_refuses_bad_cubes_and_weights_before_any_context(pkg):
    ws = pkg.TransformBuilder.new().build_merging()
    good = np.zeros((2, 8, 8), dtype=np.uint8)
    with pytest.raises(ValueError):
        ws.merge_tree_stats_cube(np.zeros((8, 8), dtype=np.uint8))                       # not 3-D
    with pytest.raises(ValueError):
        ws.merge_tree_stats_cube(np.zeros((2, 3, 8, 8), dtype=np.uint8))
    with pytest.raises(ValueError):
        ws.merge_tree_stats_cube(np.zeros((3, 8, 8), dtype=np.uint8), seeds=[[(1, 1)], [(2, 2)]])      # two lists, three slices
    with pytest.raises(ValueError):
        ws.merge_tree_stats_cube(np.zeros((2, 8, 8), dtype=np.float32))                  # not u8
    with pytest.raises(ValueError):
        ws.merge_tree_stats_cube(good, weights=np.zeros((2, 8, 9), dtype=np.uint8))      # another shape
    with pytest.raises(ValueError):
        ws.merge_tree_stats_cube(good, weights=np.zeros((3, 8, 8), dtype=np.uint16))
    with pytest.raises(TypeError):
        ws.merge_tree_stats_cube(good, weights=np.zeros((2, 8, 8), dtype=np.float32))    # not u8 / u16
    with pytest.raises(TypeError):
        ws.merge_tree_stats_cube(good, weights=np.zeros((8, 8), dtype=np.uint8))         # a plane, not a cube


def test_segmenting_wrapper_has_no_stats_cube(pkg):
    assert hasattr(pkg.MergingWatershed, "merge_tree_stats_cube") and not hasattr(pkg.SegmentingWatershed, "merge_tree_stats_cube")


# ---- the GPU tests' inputs reach their regimes ----------------------------------------------------------------------------------

def test_all_255_steps_hold_uncoloured_pixels_of_two_slices_and_a_seed():
    shape, lists = bc.all_255_case("last_rows")
    s, h, w = shape
    plane = h * w
    assert plane % bc.STEP != 0 and plane % 128 == 0 and plane % 4 == 0      # steps straddle slices, quads do not
    assert all(2 <= len(l) <= 3 for l in lists)
    seeded = np.zeros(s * plane, dtype=bool)
    for k, l in enumerate(lists):
        seeded[k * plane + l[:, 0] * w + l[:, 1]] = True
    slice_of = np.arange(s * plane) // plane
    hits = 0
    for p0 in range(0, s * plane, bc.STEP):
        run = slice(p0, min(p0 + bc.STEP, s * plane))
        unc = np.unique(slice_of[run][~seeded[run]])
        if unc.size == 2 and seeded[run].any():
            hits += 1
    assert hits >= 2, hits
    # seeds of slices 1 and 2 lie in the last rows: in the step that also holds the next slice's first pixels
    for k, rows in ((1, slice(0, 3)), (2, slice(1, 3))):
        last = (k * plane + lists[k][rows, 0] * w + lists[k][rows, 1]) // bc.STEP
        assert ((k + 1) * plane) % bc.STEP != 0 and (last == ((k + 1) * plane) // bc.STEP).all(), k
    # checkerboard: a workgroup's step of 1024 pixels holds 512 seeds and 512 uncoloured pixels of one slice: 513 keys, 512 slots
    shape, lists = bc.all_255_case("checkerboard")
    s, h, w = shape
    assert h * w == 2 * bc.STEP
    for l in lists:
        idx = l[:, 0] * w + l[:, 1]
        assert len(l) == 1024 and (np.bincount(idx // bc.STEP) == 512).all()
    # the closed form is what the oracle route gives
    img = np.full((h, w), 255, dtype=np.uint8)
    wt = bc.weight_cubes(shape, 77)[2][1]
    tree, want = ls.expected(img, lists[0][:40], wt[0])
    assert ls.mismatch(bc.all_255_expected(wt[0], lists[0][:40]), want) is None
    assert (tree[1:, 1] == mt.ALIVE).all() and (tree[1:, 2] == 1).all() and tree[0, 2] == h * w - 40


def test_level_zero_death_case_kills_a_colour_at_level_0_in_later_slices():
    imgs, lists, dying = bc.level_zero_death_case()
    assert [k for k, _ in dying] == [1, 3]
    for k, c in dying:
        for edge, shift in ((False, False), (True, True)):
            parent, death, area, leaves, vals, ex = mt.expected_tree(imgs[k], lists[k], 254, edge, shift)
            assert death[c] == 0 and leaves[c] == 1 and area[c] == 1 and 0 < parent[c] < c, (k, c, edge)
        assert (np.diff(lists[k][:, 0] * 96 + lists[k][:, 1]) > 0).all()      # strictly row-major: the stack is taken


def test_random_cases_have_distinct_records_zero_and_one_case_has_the_identity():
    """Record 0 of a slice of a random field is never the identity: the border of a plane is never flooded.  So the random cases
    prove that the seedless slice's record 0 (its whole plane) differs from its neighbours' (their borders, and whatever holds
    255), and that without edge correction -- where the border carries the slice's own weights -- all three differ: one slice's
    uncoloured pixels landing in another's record shows.  With edge correction the border is the ring of zeros, the same in every
    slice.  The identity is reached by empty_record_zero_case, whose middle slice has no uncoloured pixel."""
    for shape, edge in bc.SHAPES[:3]:
        imgs = bc.random_images(shape)
        lists = bc.seed_lists(imgs)
        wt = bc.weight_cubes(shape, 40)[2][1]
        zeros = []
        for k in (0, 1, 2):
            tree, rec = ls.expected(imgs[k], lists[k], wt[k], 254, edge)
            assert rec[0] != ls.empty_records(1)[0] and tree[0][2] > 0
            zeros.append(rec[0])
        assert zeros[0] != zeros[1] and zeros[1] != zeros[2] and (edge or zeros[0] != zeros[2])
        assert int(zeros[1]["sum_r"]) == (shape[2] + (2 if edge else 0)) * sum(range(shape[1] + (2 if edge else 0)))      # the seedless slice: all of it
    imgs, lists, full = bc.empty_record_zero_case()
    wt = bc.weight_cubes((3, 8, 16), 46)[2][1]
    assert imgs[0].size % 128 == 0
    for k in range(3):
        tree, rec = ls.expected(imgs[k], lists[k], wt[k])
        assert (rec[0] == ls.empty_records(1)[0]) == (k == full), k
        assert (tree[0][2] == 0) == (k == full), k
