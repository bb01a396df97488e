"""Layouts for the strided-input tests: an image (or a cube of slices) embedded in a larger flat byte array, as a caller's
ArrayView2<u8> into a bigger allocation is.  Every byte that is not a pixel -- the guard bands before and after, the gaps
between rows and between slices -- holds `fill`: 0x00 (ALWAYS_FILL: a stray read floods early), 0xFF (NEVER_FILL: a stray
read never floods) or, with fill="random" / ("random", seed), a seeded random stream."""
import numpy as np

GUARD = 4096


def _backing(n, fill):
    if isinstance(fill, tuple) or fill == "random":
        seed = fill[1] if isinstance(fill, tuple) else 0
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    if fill not in (0x00, 0xFF):
        raise ValueError("fill is 0x00, 0xFF, 'random' or ('random', seed)")
    return np.full(n, fill, dtype=np.uint8)


def plane_bytes(h, w, offset, row_stride, guard=GUARD):
    """Size of embed()'s backing array: the last row owns only w bytes."""
    return guard + offset + (max(h, 1) - 1) * row_stride + w + guard


def embed(img, offset, row_stride, fill, guard=GUARD):
    """(backing, off, mask): flat uint8 backing array with pixel (y, x) at off + y * row_stride + x, off = guard + offset;
    mask is True at every byte that is not a pixel."""
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape
    if row_stride < w or offset < 0:
        raise ValueError("row_stride >= w and offset >= 0")
    backing = _backing(plane_bytes(h, w, offset, row_stride, guard), fill)
    mask = np.ones(backing.size, dtype=bool)
    off = guard + offset
    for y in range(h):
        backing[off + y * row_stride: off + y * row_stride + w] = img[y]
        mask[off + y * row_stride: off + y * row_stride + w] = False
    return backing, off, mask


def cube_bytes(s, h, w, offset, row_stride, slice_stride, guard=GUARD):
    return guard + offset + (max(s, 1) - 1) * slice_stride + (max(h, 1) - 1) * row_stride + w + guard


def embed_cube(cube, offset, row_stride, slice_stride, fill, guard=GUARD):
    """The same for a cube (s, h, w): pixel (k, y, x) at off + k * slice_stride + y * row_stride + x."""
    cube = np.asarray(cube, dtype=np.uint8)
    s, h, w = cube.shape
    if row_stride < w or offset < 0 or (s > 1 and slice_stride < (h - 1) * row_stride + w):
        raise ValueError("row_stride >= w, offset >= 0 and slices that do not overlap")
    backing = _backing(cube_bytes(s, h, w, offset, row_stride, slice_stride, guard), fill)
    mask = np.ones(backing.size, dtype=bool)
    off = guard + offset
    for k in range(s):
        for y in range(h):
            p = off + k * slice_stride + y * row_stride
            backing[p: p + w] = cube[k, y]
            mask[p: p + w] = False
    return backing, off, mask


def view(backing, off, h, w, row_stride):
    """The numpy view of the embedded plane: shape (h, w), strides (row_stride, 1)."""
    return np.lib.stride_tricks.as_strided(backing[off:], shape=(h, w), strides=(row_stride, 1), writeable=False)


def view_cube(backing, off, s, h, w, row_stride, slice_stride):
    return np.lib.stride_tricks.as_strided(backing[off:], shape=(s, h, w), strides=(slice_stride, row_stride, 1), writeable=False)


def row_stride_of(kind, w):
    """The row strides the strided-input tests name."""
    if kind == "w":
        return w
    if kind in ("w+1", "w+2", "w+3", "w+4"):
        return w + int(kind[2:])
    if kind == "pitch":
        return (w + 255) // 256 * 256
    if kind == "2w":
        return 2 * w
    raise ValueError(kind)
