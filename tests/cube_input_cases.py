"""Inputs of the cube front end's tests (tests/test_cube_input_cases_cpu.py on the CPU, tests/test_gpu_cube_input.py on the GPU):
built from numpy alone, so that the CPU tests can prove what the cubes are claimed to contain before a kernel sees them.

The kernels' geometry these cases are laid out against (rustronomy-watershed_amd/csrc/ws_cube_input.hip, ws_kernels.hip):
  channel-last tiles   a wave holds SL = 8, 16, 32 or 64 (= CL_S) slices, the smallest that holds the cube's, by 64 / SL pixels; a
                       workgroup's tile is SL slices x CL_P * 64 / SL = 1024, 512, 256 or 128 (= CL_P) pixels; lanes are
                       (pixel, slice) pairs on the load side and lie along the pixels (4 bytes a lane) on the store side
  rows / gather        256 threads a workgroup, workgroup (slice, part) walks the pixels part * 256 + t, + B * 256, ...
  stacked minima       strips of 8 stacked rows, segments of 1024 columns, one wave per stacked row in the write pass
"""
import numpy as np

CL_P, CL_S = 128, 64
MID, LOW, HIGH = 1, -3, 5
SIGNED = ("float64", "float32", "int32", "int16")
UNSIGNED = ("uint8", "uint16")
DTYPES = SIGNED + UNSIGNED

K_SET = (1, 2, 7, 8, 9, 16, 17, 32, 33, 63, 64, 65, 130)   # both sides of every wave shape's edge: 8, 16, 32, CL_S
PLANES = ((1, 1), (1, 255), (255, 1), (1, 256), (256, 1), (1, 257), (257, 1), (1, 1025), (1025, 1), (5, 205),
          (1, CL_P - 1), (1, CL_P), (1, CL_P + 1), (1, 511), (1, 513), (1, 1023))
# h * w in {1, 255, 256, 257, 1025} and both sides of every tile's pixel count: 128, 256, 512, 1024
LAYOUTS = ("contiguous", "channel_last", "strided")


def placed_indices(hw):
    return [i for i in sorted({0, 1, 63, 64, CL_P - 1, CL_P, CL_P + 1, 255, 256, hw - 2, hw - 1}) if 0 <= i < hw]


def slice_extremes(k, n_slices, dtype):
    """(low, high) of slice k: pairwise different between slices; the cube's lowest value lies in the LAST slice and its highest in
    the FIRST, so that (two slices or more, signed) no slice has the whole cube's (min, max)."""
    low = LOW - k if dtype in SIGNED else None
    high = HIGH + (n_slices - 1 - k) if dtype in SIGNED else HIGH + k
    return low, high


def preproc_cube(n_slices, h, w, dtype, flank=False):
    """(n_slices, h, w): every slice a ramp 1, 2, 3, 1, ... with its own unique minimum and maximum (slice_extremes) at positions of
    placed_indices that move with the slice: the first and the last pixel and both sides of every tile edge occur.  A one-pixel
    slice holds its maximum alone (even k) or its minimum (odd k, signed).  flank (float): NaN, +inf, -inf beside the extremes."""
    hw = h * w
    cube = np.empty((n_slices, hw), dtype=dtype)
    idx = placed_indices(hw)
    for k in range(n_slices):
        a = (1 + np.arange(hw) % 3).astype(dtype)
        low, high = slice_extremes(k, n_slices, dtype)
        p, q = idx[k % len(idx)], idx[(k + len(idx) // 2) % len(idx)]
        if q == p:
            q = idx[(k + 1) % len(idx)]
        if hw == 1:
            a[0] = high if (k % 2 == 0 or low is None) else low
        else:
            a[q] = high
            if low is not None:
                a[p] = low
            if flank:
                specials = [np.nan, np.inf, -np.inf, np.nan]
                j = 0
                for centre in (p, q):
                    for d in (-1, 1):
                        at = centre + d
                        if 0 <= at < hw and at not in (p, q):
                            a[at] = specials[j % 4]
                            j += 1
        cube[k] = a
    return cube.reshape(n_slices, h, w)


def lay_out(cube, layout):
    """A view equal to `cube` (slices, rows, columns) over storage of the given layout.  `strided` is a [::2, ::3, ::2] view of a
    larger array whose other elements hold values beyond every slice's extremes: a kernel that reads one changes every byte."""
    n, h, w = cube.shape
    if layout == "contiguous":
        return np.ascontiguousarray(cube)
    if layout == "channel_last":
        store = np.ascontiguousarray(np.moveaxis(cube, 0, -1))      # (h, w, n): the slice index is the last axis
        return np.moveaxis(store, -1, 0)
    assert layout == "strided"
    filler = 250 if cube.dtype == np.uint8 else 20000
    store = np.full((2 * n, 3 * h, 2 * w + 3), filler, dtype=cube.dtype)
    if cube.dtype.name in SIGNED:
        store[1::2] = -filler
    view = store[::2, ::3, :2 * w:2]
    view[...] = cube
    return view


def element_strides(view):
    return tuple(s // view.dtype.itemsize for s in view.strides)


def seeded_minmax(cube):
    """numpy's zero-seeded folds of every slice (lib.rs:1147-1156): (n_slices, 2) float64."""
    out = np.zeros((cube.shape[0], 2))
    for k, s in enumerate(cube):
        x = s.astype(np.float64).reshape(-1)
        x = x[np.isfinite(x)]
        out[k] = (min(0.0, x.min()) if x.size else 0.0, max(0.0, x.max()) if x.size else 0.0)
    return out


def rounding_cube(dtype, r, lo):
    """The rounding ramps of preproc_cases.rounding_cases() as slices: slice k is the ramp lo .. lo + r rotated by k, so every slice
    has the same (min, max) = (min(lo, 0), lo + r) at its own positions; 3 slices of r + 1 pixels."""
    v = np.arange(lo, lo + r + 1, dtype=np.int64)
    return np.stack([np.roll(v, 17 * k) for k in range(3)]).astype(dtype).reshape(3, 1, r + 1)


def overflow_cube():
    """f64, 7 slices of 2 x 3: slices 3 and 5 span more than DBL_MAX, the others do not.  near_miss: the same cube with +-8.9e307 in
    their place, a finite range."""
    cube = np.tile(np.array([[1.0, -3.0, 5.0], [2.0, np.nan, 0.5]]), (7, 1, 1)) * (1 + np.arange(7))[:, None, None]
    near = cube.copy()
    for k, (at_lo, at_hi) in ((3, ((0, 1), (1, 2))), (5, ((1, 0), (0, 0)))):
        cube[k][at_lo], cube[k][at_hi] = -1e308, 1e308
        near[k][at_lo], near[k][at_hi] = -8.9e307, 8.9e307
    return cube, near


# ---- minima -------------------------------------------------------------------------------------------------------------------

LOW_BORDER = 2      # the slice of border_maxima_cube whose own border rows are low


def border_maxima_cube(n_slices=5, h=5, w=37, seed=11):
    """Every slice but LOW_BORDER: rows 0 and h - 1 hold 200 (row 0) and 200 / 220 alternating (row h - 1), above everything in the
    rows next to them in their own slice (< 100) and in the neighbouring slice: in the STACKED plane the 220s of a last row are strict
    maxima, in their slice they are border pixels.  Slice LOW_BORDER has zero border rows and planted maxima (150) on its rows 1 and
    h - 2, which a clamp to the stack's rows instead of the slice's would hide behind its neighbours' 200s."""
    rng = np.random.default_rng(seed)
    cube = rng.integers(0, 100, size=(n_slices, h, w), dtype=np.uint8)
    cube[:, 0, :] = 200
    cube[:, h - 1, :] = 200
    cube[:, h - 1, 1::2] = 220
    cube[LOW_BORDER, 0, :] = 0
    cube[LOW_BORDER, h - 1, :] = 0
    cube[LOW_BORDER, 1, 2::4] = 150
    cube[LOW_BORDER, h - 2, 4::4] = 150
    return cube


def seedless_cube(n_slices=5, h=6, w=9, seed=5):
    """Random slices; the first, the middle and the last are constant: no seeds, their offsets repeat."""
    rng = np.random.default_rng(seed)
    cube = rng.integers(0, 255, size=(n_slices, h, w), dtype=np.uint8)
    for k in (0, n_slices // 2, n_slices - 1):
        cube[k] = 7
    return cube


def lattice_cube(n_slices=3, h=9, w=13):
    """Every 2 x 2 block of every slice's interior holds a maximum: (h - 1) // 2 * ((w - 1) // 2) a slice, the most a slice can hold."""
    cube = np.zeros((n_slices, h, w), dtype=np.uint8)
    cube[:, 1:h - 1:2, 1:w - 1:2] = 200
    cube += (np.arange(n_slices, dtype=np.uint8) * 3)[:, None, None]
    return cube


def lattice_count(n_slices, h, w):
    return n_slices * ((h - 1) // 2) * ((w - 1) // 2)


MINIMA_H = (1, 2, 3, 5, 8, 9, 13)
MINIMA_W = (2, 3, 5, 32, 33, 1028, 2052)


def random_cube(n_slices, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n_slices, h, w), dtype=np.uint8)


def per_slice_minima(cube, find):
    """(seeds (n, 2) uint64, offsets (n_slices + 1) uint64) from `find` (a single-plane find_local_minima) slice by slice."""
    lists = [np.asarray(find(np.ascontiguousarray(s)), dtype=np.uint64).reshape(-1, 2) for s in cube]
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    seeds = np.concatenate(lists) if lists else np.zeros((0, 2), np.uint64)
    return seeds.reshape(-1, 2), offsets
