"""The layout helper of the strided-input GPU tests (tests/strided.py), checked on the CPU."""
import numpy as np
import pytest

import __graft_entry__ as ge
import strided

STRIDES = ["w", "w+1", "w+2", "w+3", "w+4", "pitch", "2w"]


@pytest.mark.parametrize("fill", [0x00, 0xFF, "random", ("random", 7)])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 3), (31, 96), (7, 520)])
def test_embed_plane(h, w, fill):
    img = np.random.default_rng(h * 1000 + w).integers(1, 255, (h, w), dtype=np.uint8)
    for offset in (0, 1, 2, 3, 4, 64):
        for kind in STRIDES:
            rs = strided.row_stride_of(kind, w)
            backing, off, mask = strided.embed(img, offset, rs, fill)
            assert backing.dtype == np.uint8 and backing.ndim == 1 and off == strided.GUARD + offset
            assert backing.size == strided.GUARD + offset + (h - 1) * rs + w + strided.GUARD == strided.plane_bytes(h, w, offset, rs)
            v = strided.view(backing, off, h, w, rs)
            assert v.strides == (rs, 1) and (v == img).all()
            # the mask marks exactly the bytes that are not pixels
            want = np.ones(backing.size, dtype=bool)
            idx = (off + np.arange(h)[:, None] * rs + np.arange(w)[None, :]).ravel()
            want[idx] = False
            assert (mask == want).all() and int((~mask).sum()) == h * w
            assert mask[:off].all() and mask[off + (h - 1) * rs + w:].all()
            if fill in (0x00, 0xFF):
                assert (backing[mask] == fill).all()
            else:
                again, _, _ = strided.embed(img, offset, rs, fill)
                assert (again == backing).all()                      # seeded: the same stream every time
                if mask.sum() > 64:
                    assert len(np.unique(backing[mask])) > 8


def test_embed_small_guard_and_bad_arguments():
    img = np.arange(12, dtype=np.uint8).reshape(3, 4)
    backing, off, mask = strided.embed(img, 3, 9, 0xFF, guard=16)
    assert backing.size == 16 + 3 + 2 * 9 + 4 + 16 and off == 19
    assert (strided.view(backing, off, 3, 4, 9) == img).all()
    with pytest.raises(ValueError):
        strided.embed(img, 0, 3, 0x00)
    with pytest.raises(ValueError):
        strided.embed(img, 0, 4, 0x55)
    with pytest.raises(ValueError):
        strided.embed_cube(np.zeros((2, 3, 4), np.uint8), 0, 5, 13, 0x00)      # the slices would overlap


@pytest.mark.parametrize("fill", [0x00, 0xFF, "random"])
def test_embed_cube(fill):
    s, h, w = 4, 6, 10
    cube = np.random.default_rng(3).integers(1, 255, (s, h, w), dtype=np.uint8)
    for offset, rs, ss in ((0, 13, 6 * 13), (1, 10, 61), (3, 10, 70), (2, 12, 6 * 12 + 12), (5, 10, 60)):
        backing, off, mask = strided.embed_cube(cube, offset, rs, ss, fill)
        assert backing.size == strided.GUARD + offset + (s - 1) * ss + (h - 1) * rs + w + strided.GUARD
        v = strided.view_cube(backing, off, s, h, w, rs, ss)
        assert v.strides == (ss, rs, 1) and (v == cube).all()
        want = np.ones(backing.size, dtype=bool)
        idx = off + np.arange(s)[:, None, None] * ss + np.arange(h)[None, :, None] * rs + np.arange(w)[None, None, :]
        want[idx.ravel()] = False
        assert (mask == want).all()
        if fill != "random":
            assert (backing[mask] == fill).all()
        for k in range(s):      # every slice is the plane helper's view at its own base
            assert (strided.view(backing, off + k * ss, h, w, rs) == cube[k]).all()


def test_api_accepts_the_view_with_its_stride():
    api = ge.load_package().api
    img = np.random.default_rng(1).integers(0, 255, (9, 20), dtype=np.uint8)
    for offset, kind in ((1, "w+3"), (0, "pitch"), (2, "2w"), (3, "w")):
        rs = strided.row_stride_of(kind, 20)
        backing, off, _ = strided.embed(img, offset, rs, 0xFF)
        v = strided.view(backing, off, 9, 20, rs)
        a, stride = api._as_image(v)
        assert stride == rs and a.ctypes.data == backing.ctypes.data + off and (a == img).all()
