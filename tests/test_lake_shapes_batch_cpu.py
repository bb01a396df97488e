"""merge_tree_shapes of a cube without a GPU: the new symbols at the boundary and the proof that the cubes of
tests/lake_shapes_batch_cases.py reach the regimes tests/test_gpu_lake_shapes_batch.py names -- stacks and loops, steps that
straddle slices, slices that differ, the 128-bit high word on a plane that is not FLAT, more roots in a step than the table has
slots with colours of two slices among them, a level-0 death in a later slice and an empty record 0."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import lake_shapes_batch_cases as sbc
import lake_shapes_cases as lc
import lake_shapes_ref as sh
import lake_stats_batch_cases as bc
import merge_tree_ref as mt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ws_merge_tree_shapes_batch_device", "ws_merge_tree_shapes_batch")


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


# ---- (f) the boundary -------------------------------------------------------------------------------------------------------------------

def test_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "ws_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(pkg._ffi.LIB_PATH)
    ffi_rs = open(os.path.join(ROOT, "rust", "src", "hip_ffi.rs")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in pkg._ffi.SIGNATURES
        assert getattr(raw, name) is not None
        assert re.search(r"\bfn\s+" + name + r"\s*\(", ffi_rs), name
    assert pkg._ffi.lib().ws_abi_version() == pkg._ffi.WS_ABI_VERSION == 3
    assert pkg.api.LAKE_SHAPE_DTYPE.itemsize == 96
    assert "merge_tree_shapes_cube" in open(os.path.join(ROOT, "rust", "src", "watershed_hip.rs")).read()
    assert "merge_tree_shapes_cube" in open(os.path.join(ROOT, "include", "ws_watershed.hpp")).read()
    assert hasattr(pkg.MergingWatershed, "merge_tree_shapes_cube") and not hasattr(pkg.SegmentingWatershed, "merge_tree_shapes_cube")
    device = open(os.path.join(ROOT, "rustronomy-watershed_amd", "device.py")).read()
    assert "def merge_tree_shapes_batch(" in device


def test_null_context_is_bad_arg(pkg):
    L = pkg._ffi.lib()
    opt = pkg._ffi.Options()
    buf = np.zeros(64, dtype=np.uint64)
    offs = (ctypes.c_size_t * 2)(0, 1)
    p, o = buf.ctypes.data, ctypes.byref(opt)
    assert L.ws_merge_tree_shapes_batch_device(None, p, 1, 4, 4, 4, 16, p, offs, o, None, 0, 0, 0, p, p, p, None, None) == pkg._ffi.WS_ERR_BAD_ARG
    assert L.ws_merge_tree_shapes_batch(None, p, 1, 4, 4, 4, 16, p, offs, o, None, 0, 0, 0, p, p, p, 2, None, None, None, None) == pkg._ffi.WS_ERR_BAD_ARG


# ---- (a) stacks, loops and straddling steps ---------------------------------------------------------------------------------------------

def test_three_shapes_stack_two_loop_and_a_step_straddles_two_slices():
    stacked = [sbc.cube(f"shape:{i}:image").stacks() for i in range(len(bc.SHAPES))]
    assert stacked == [True, True, True, False, False]
    for i in range(len(bc.SHAPES)):
        c = sbc.cube(f"shape:{i}:u16")
        assert len(c.lists[1]) == 0 and len(c.lists[2]) == 1 and all(len(l) > 1 for l in c.lists[3:])
    c = sbc.cube("shape:2:u16")
    assert c.shape == (5, 40, 96)
    ph, pw = c.plane
    plane = ph * pw
    assert plane % 4 == 0                       # a quad never straddles
    straddling = [i for i in range(0, c.shape[0] * plane, sbc.STEP) if i // plane != min(i + sbc.STEP - 1, c.shape[0] * plane - 1) // plane]
    assert straddling and straddling[0] == 3 * sbc.STEP          # pixels 3072 .. 4095 hold the end of slice 0 and the start of slice 1


@pytest.mark.parametrize("name", ["shape:0:u16", "shape:2:u8", "differ"])
def test_reference_of_a_slice_is_lake_shapes_refs(name):
    """SliceRef derives tree, stats and sums from one oracle run: the same as lake_shapes_ref.expected on the slice alone."""
    c = sbc.cube(name)
    for k, r in enumerate(sbc.reference(name)):
        tree, stats, sums = sh.expected(c.imgs[k], c.lists[k], c.slice_weights(k), c.max_level, c.edge, c.seed_shift)
        assert (r.tree == tree).all() and (r.stats == stats).all() and (r.sums == sums).all(), k
    first = c.first()
    want = sbc.expected_sums(name)
    assert len(want) == first[-1] == sum(len(l) for l in c.lists) + len(c.imgs)
    for k, r in enumerate(sbc.reference(name)):
        assert (want[first[k]:first[k + 1]] == r.sums).all()


# ---- (b) slices that differ -------------------------------------------------------------------------------------------------------------

def test_a_colour_differs_between_slice_0_and_slice_1_in_all_six_sums():
    r0, r1 = sbc.reference("differ")[:2]
    n = min(len(r0.sums), len(r1.sums))
    every = [c for c in range(1, n) if all(r0.sums[c, j] != r1.sums[c, j] for j in range(6))]
    assert every, "no colour tells slice 0 from slice 1 in every sum"
    # that colour holds pixels in slice 1: with stacked rows (row + ph) its sum of row^2 would grow by 2 ph sum_r + area ph^2 > 0
    assert int(r1.tree[every[0], 2]) > 0 and sbc.cube("differ").plane[0] > 0
    # and the weight planes of the two slices differ where it matters: a kernel that read slice 0's weights for slice 1 would not
    # reproduce slice 1's weighted sums from its plain ones
    wt = sbc.cube("differ").weights
    assert (wt[0] != wt[1]).mean() > 0.9


# ---- (c) the high word on a plane that is not FLAT --------------------------------------------------------------------------------------

def test_high_word_cube_stacks_is_not_flat_and_passes_64_bits_in_every_slice():
    s, h, w = sbc.HIGH_SHAPE
    c = sbc.cube("high_word")
    assert c.stacks() and (h * w) % 128 == 0 and w % 4 == 0
    assert max(h, w) >= 65536                                  # FLAT is decided from a slice's sides: the wave join moves twelve limbs
    assert s * h < 65536                                       # ... and not from the stacked height, which would say the same here
    wt = sbc.high_word_weights()
    assert wt.dtype == np.uint16 and int(wt.min()) > 65000
    assert lc.accepted(h, w, int(wt.max()))                    # the stats call's bound takes the plane
    for k in range(s):
        tree, sums = sbc.high_word_expected(k)
        assert sums[1][1] >= 1 << 64, k                          # the sum of v col^2 over the slice's lake
        assert all(x < 1 << 96 for row in sums for x in row)
        assert tree[:, 2].sum() == h * w
        r, x = sbc.HIGH_SEEDS[k]
        assert 0 < r < h - 1 and 0 < x < w - 1                  # the seed is in the interior: it floods all of it at level 0
    a, b = sbc.high_word_expected(0)[1], sbc.high_word_expected(1)[1]
    assert all(a[1][j] != b[1][j] for j in range(3)) and all(a[1][j] == b[1][j] for j in range(3, 6))


def test_rect_sums_against_the_terms_of_a_small_plane():
    h, w = 8, 40
    rows = [65535 - r for r in range(h)]
    v = np.repeat(np.array(rows, dtype=np.int64)[:, None], w, axis=1)
    T = sh.terms(v)
    inside = np.zeros((h, w), dtype=np.int64)
    inside[1:-1, 1:-1] = 1
    brute = sh.sums_by_key(inside.ravel(), T, np.arange(h * w), 2)
    assert brute[1].tolist() == sbc.rect_sums(rows, 1, h - 1, 1, w - 1)
    assert (brute[0] + brute[1]).tolist() == sbc.rect_sums(rows, 0, h, 0, w)
    assert sbc.rect_sums([255] * 3, 0, 3, 0, 1000) == sh.closed_form_line_plane(3, 1000, 255)


# ---- (d) colours of two slices in one table ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["all_seeds", "all255:small_checkerboard", "all255:last_rows", "all255:checkerboard"])
def test_a_step_meets_more_roots_than_slots_or_roots_of_two_slices(name):
    """all_seeds does NOT overflow the table, whatever its 384 seeds suggest: seeds are coloured before level 0, so seeds that
    touch are one lake from level 0 on and every interior pixel has the same root; only the border seeds (never paired) keep
    their own.  The cube still puts the same own colours of three slices into one step.  The overflow with several slices in
    the step comes from all255:small_checkerboard, whose seeds never touch."""
    steps = sbc.step_owners(name)
    slots = lc.table_slots()
    most = max(len(s) for s in steps)
    two = [s for s in steps if len({k for k, c in s if c != 0}) > 1]          # colours (not record 0) of two slices in one step
    if name == "all_seeds":
        assert len(steps) == 1 and two and most < slots, (most, slots)
        # the same own colour from two slices in that step: a table keyed by a slice's own colour would join them
        assert any((0, c) in steps[0] and (1, c) in steps[0] for c in range(1, 129))
        assert sum(int((r.death[1:] == 0).sum()) for r in sbc.reference(name)) > 3 * 60      # the interior seeds die at level 0
    elif name == "all255:small_checkerboard":
        assert len(steps) == 1 and most == 8 * 65 > slots and two
        assert all((k, c) in steps[0] for k in range(8) for c in range(65))      # every own colour, and record 0, from every slice
    elif name == "all255:checkerboard":
        assert all(len(s) == 513 for s in steps) and 513 > slots and not two
    else:
        assert two, "no step holds seeds of two slices"
        assert any({k for k, c in s if c == 0} >= {0, 1} for s in steps)          # and uncoloured pixels of two slices


# ---- (e) special records ----------------------------------------------------------------------------------------------------------------

def test_level_zero_death_in_a_later_slice_and_an_empty_record_zero():
    _, _, dying = bc.level_zero_death_case()
    for name in ("level0", "level0:edge"):
        refs = sbc.reference(name)
        assert dying and all(k >= 1 for k, _ in dying)
        for k, c in dying:
            assert refs[k].tree[c, 1] == 0 and refs[k].tree[c, 3] == 1
    _, _, full = bc.empty_record_zero_case()
    refs = sbc.reference("empty0")
    assert full == 1 and sbc.cube("empty0").stacks()
    for k, r in enumerate(refs):
        assert (not any(r.sums[0])) == (k == full) and (r.tree[0, 2] == 0) == (k == full), k
