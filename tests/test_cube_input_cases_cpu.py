"""What tests/cube_input_cases.py claims about its cubes, proved on the CPU with the oracle, and the binding tables of the cube
front end (ws_pre_processor_batch(_device), ws_find_local_minima_batch(_device))."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import cube_input_cases as cc
import oracle_lib as ol
import preproc_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ws_pre_processor_batch_device", "ws_pre_processor_batch", "ws_find_local_minima_batch_device", "ws_find_local_minima_batch")


def test_sets_cover_both_tile_axes():
    assert {cc.CL_S - 1, cc.CL_S, cc.CL_S + 1, 1, 2, 130} <= set(cc.K_SET)
    for sl in (8, 16, 32):                                           # the wave shapes for few slices, and their tiles' pixel counts
        assert {sl, sl + 1} <= set(cc.K_SET)
        tp = cc.CL_P * 64 // sl
        assert {tp - 1, tp + 1} <= {h * w for h, w in cc.PLANES}
    sizes = {h * w for h, w in cc.PLANES}
    assert {1, 255, 256, 257, 1025, cc.CL_P - 1, cc.CL_P, cc.CL_P + 1} <= sizes
    for n in (255, 256, 257, 1025):
        assert (1, n) in cc.PLANES and (n, 1) in cc.PLANES
    assert (5, 205) in cc.PLANES
    text = open(os.path.join(ROOT, "rustronomy-watershed_amd", "csrc", "ws_cube_input.hip")).read()
    assert re.search(r"constexpr int CL_P = (\d+);", text).group(1) == str(cc.CL_P)
    assert re.search(r"constexpr int CL_S = (\d+);", text).group(1) == str(cc.CL_S)


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("plane", [(1, 255), (5, 205), (1, cc.CL_P + 1)])
def test_every_slice_needs_its_own_extremes(dtype, plane):
    """A kernel that folds (min, max) over the whole cube gets EVERY slice wrong (unsigned: every slice but the one holding the
    cube's maximum -- their minimum is the folds' seed 0 everywhere)."""
    for n in (2, 5, 65):
        cube = cc.preproc_cube(n, *plane, dtype)
        mm = cc.seeded_minmax(cube)
        assert len({tuple(r) for r in mm}) == n                      # pairwise different (min, max)
        whole = ol.pre_processor(cube)
        same = [k for k in range(n) if (ol.pre_processor(np.ascontiguousarray(cube[k])) == whole[k]).all()]
        assert same == ([] if dtype in cc.SIGNED else [n - 1]), (dtype, n, same)
        # the extremes sit where claimed: first pixel, last pixel and both sides of a tile edge occur among the slices
        flat = cube.reshape(n, -1)
        at_max = {int(np.argmax(s)) for s in flat}
        assert at_max <= set(cc.placed_indices(flat.shape[1]))
        if n >= 11:
            assert {0, flat.shape[1] - 1, cc.CL_P - 1, cc.CL_P} <= at_max


def test_layouts_are_views_of_the_same_cube():
    cube = cc.preproc_cube(5, 5, 7, "float32", flank=True)
    for layout in cc.LAYOUTS:
        v = cc.lay_out(cube, layout)
        assert v.shape == cube.shape and np.array_equal(v, cube, equal_nan=True)
        ss, rs, cs = cc.element_strides(v)
        if layout == "channel_last":
            assert (ss, rs, cs) == (1, 7 * 5, 5)
        if layout == "strided":
            assert rs > 7 * cs and cs == 2 and min(ss, rs, cs) > 0
            assert np.nanmax(np.abs(np.where(np.isinf(v.base), 0, v.base))) == 20000                     # what lies between the view's elements would move every fold
    assert np.isnan(cube).any() and np.isinf(cube).any()


def test_rounding_and_overflow_cubes():
    assert any(a.size == 254 for _, a in pc.rounding_cases())
    cube = cc.rounding_cube("float64", 253, 0)
    assert cube.shape == (3, 1, 254) and all(sorted(s.reshape(-1)) == list(range(254)) for s in cube)
    bad, near = cc.overflow_cube()
    for k in range(7):
        if k in (3, 5):
            with pytest.raises(ol.ReferencePanics):
                ol.pre_processor(np.ascontiguousarray(bad[k]))
        else:
            ol.pre_processor(np.ascontiguousarray(bad[k]))
        ol.pre_processor(np.ascontiguousarray(near[k]))
    with np.errstate(over="ignore"):
        as32 = bad.astype(np.float32)
    assert np.isinf(as32[3]).sum() == 2


def test_border_maxima_cube_tells_a_stack_clamp_from_a_slice_clamp():
    cube = cc.border_maxima_cube()
    n, h, w = cube.shape
    seeds, offsets = cc.per_slice_minima(cube, ol.find_local_minima)
    stacked = np.asarray(ol.find_local_minima(cube.reshape(n * h, w)), dtype=np.uint64).reshape(-1, 2)
    as_stack = np.stack([seeds[:, 0] + np.repeat(np.arange(n, dtype=np.uint64), np.diff(offsets).astype(int)) * h, seeds[:, 1]], axis=1)
    assert not (len(stacked) == len(as_stack) and (stacked == as_stack).all())
    on_borders = [(int(r) % h) in (0, h - 1) for r, _ in stacked]
    assert any(on_borders)                                           # the stacked plane has maxima on slice borders ...
    assert not any(int(r) in (0, h - 1) for r, _ in seeds)           # ... no slice has
    for k in range(n):
        if k == cc.LOW_BORDER:
            continue
        assert cube[k, 0].min() > max(cube[k, 1].max(), cube[k - 1, h - 2].max() if k else 0)
        assert cube[k, h - 1].min() > max(cube[k, h - 2].max(), cube[k + 1, 1].max() if k + 1 < n else 0)
    mine = seeds[int(offsets[cc.LOW_BORDER]):int(offsets[cc.LOW_BORDER + 1])]
    assert 1 in mine[:, 0] and h - 2 in mine[:, 0]                   # maxima on rows 1 and h - 2 of one slice


def test_seedless_and_lattice_cubes():
    cube = cc.seedless_cube()
    n = cube.shape[0]
    seeds, offsets = cc.per_slice_minima(cube, ol.find_local_minima)
    counts = np.diff(offsets)
    assert counts[0] == counts[n // 2] == counts[-1] == 0 and counts[1] > 0 and counts[-2] > 0
    lat = cc.lattice_cube()
    seeds, offsets = cc.per_slice_minima(lat, ol.find_local_minima)
    assert len(seeds) == cc.lattice_count(*lat.shape) and len(set(np.diff(offsets))) == 1
    # no plane holds more: a strict maximum excludes its eight neighbours, one per 2 x 2 block of the interior
    h, w = lat.shape[1:]
    assert cc.lattice_count(1, h, w) == ((h - 2 + 1) // 2) * ((w - 2 + 1) // 2)


def test_minima_shapes_cross_every_path():
    assert {1, 2} <= set(cc.MINIMA_H) and any(h % 8 for h in cc.MINIMA_H) and 8 in cc.MINIMA_H      # no window; strips that straddle slices
    assert {2, 3} <= set(cc.MINIMA_W) and any(w % 4 == 0 for w in cc.MINIMA_W) and any(w % 4 for w in cc.MINIMA_W)
    assert any(1024 < w <= 2048 for w in cc.MINIMA_W) and any(2048 < w <= 3072 for w in cc.MINIMA_W)   # two and three segments


def test_bindings_declare_the_new_symbols():
    ge.build_hip()
    ffi = ge.load_package()._ffi
    header = open(os.path.join(ROOT, "include", "ws_hip.h")).read()
    mirror = open(os.path.join(ROOT, "include", "ws_watershed.hpp")).read()
    for name in NEW:
        assert name in ffi.SIGNATURES and f"int {name}(" in header
        assert getattr(ffi.lib(), name) is not None
    assert len(ffi.SIGNATURES["ws_pre_processor_batch_device"][1]) == 13 and len(ffi.SIGNATURES["ws_find_local_minima_batch_device"][1]) == 11
    assert "ws_pre_processor_batch(" in mirror and "ws_find_local_minima_batch(" in mirror
    assert ffi.WS_ABI_VERSION == 3
    pkg = ge.load_package()
    for method in ("pre_processor_cube", "pre_processor_with_max_cube", "find_local_minima_cube"):
        assert hasattr(pkg.api.WatershedUtils, method)
