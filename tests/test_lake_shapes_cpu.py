"""merge_tree_shapes without a GPU: the record's layout and the new symbols at the boundary, the reference of
tests/lake_shapes_ref.py against a second derivation, the proof that the cases of tests/lake_shapes_cases.py reach the regimes
they are there for, and api.ellipses.  The refusals that need a context are in tests/test_gpu_lake_shapes.py."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as ge
import lake_shapes_cases as lc
import lake_shapes_ref as sh
import merge_tree_ref as mt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ws_merge_tree_shapes_device", "ws_merge_tree_shapes", "ws_merge_tree_shapes_from_arrival_device")


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------

def test_record_is_96_bytes_with_the_headers_offsets(pkg):
    S = pkg._ffi.LakeShape
    assert ctypes.sizeof(S) == 96
    want = [(f, 16 * i) for i, f in enumerate(sh.FIELDS)]
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == want
    for dtype in (pkg.api.LAKE_SHAPE_DTYPE, sh.DTYPE):
        assert dtype.itemsize == 96
        assert [(f, dtype.fields[f][1]) for f in dtype.names] == want
        assert all(dtype.fields[f][0].shape == (2,) for f in dtype.names)


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
    assert "typedef struct ws_lake_shape" in code and "pub struct ws_lake_shape" in ffi_rs
    assert pkg._ffi.lib().ws_abi_version() == pkg._ffi.WS_ABI_VERSION == 3
    assert "merge_tree_shapes" in open(os.path.join(ROOT, "rust", "src", "watershed_hip.rs")).read()
    assert "merge_tree_shapes" in open(os.path.join(ROOT, "include", "ws_watershed.hpp")).read()
    assert hasattr(pkg.MergingWatershed, "merge_tree_shapes") and not hasattr(pkg.SegmentingWatershed, "merge_tree_shapes")
    assert callable(pkg.ellipses)


def test_null_context_is_bad_arg(pkg):
    L = pkg._ffi.lib()
    opt = pkg._ffi.Options()
    img = np.zeros((4, 4), dtype=np.uint8)
    seeds = np.zeros((1, 2), dtype=np.uint64)
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    o = ctypes.byref(opt)
    assert L.ws_merge_tree_shapes_device(None, img.ctypes.data, 4, 4, 4, seeds.ctypes.data, 1, o, None, 0, 0, p, p, p, None) == pkg._ffi.WS_ERR_BAD_ARG
    assert L.ws_merge_tree_shapes(None, img.ctypes.data, 4, 4, 4, seeds.ctypes.data, 1, o, None, 0, 0, p, p, p, None) == pkg._ffi.WS_ERR_BAD_ARG
    assert L.ws_merge_tree_shapes_from_arrival_device(None, p, p, 4, 4, 1, o, p, 1, 4, p, p, p) == pkg._ffi.WS_ERR_BAD_ARG


# ---- the reference ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", lc.SMALL)
def test_two_derivations_agree(name):
    r = lc.small(name)
    assert (sh.by_folding(r.planes, r.ps, r.v, r.parent, r.death, r.ex) == r.sums).all()
    # the weighted and the plain first sums come out of the same selection: lake_stats_ref's records
    T = sh.terms(r.v)
    assert sum(T[3]) == sum(int(y) ** 2 for y in range(r.v.shape[0])) * r.v.shape[1]
    # a colour that does not exist holds nothing
    gone = ~r.ex
    gone[0] = False
    assert not r.sums[gone].any()
    # the lakes alive at the end and the uncoloured pixels tile the plane
    alive = (r.death == mt.ALIVE) & r.ex
    alive[0] = True
    assert (r.sums[alive].sum(axis=0) == np.array([sum(t) for t in T], dtype=object)).all()
    assert (sh.from_words(sh.to_words(r.sums)) == r.sums).all()


def test_hand_made_records():
    """The 8 x 8 case of test_lake_stats_cpu: basins either side of a ridge, colour 3 dies at level 0 into 1, 2 at level 9."""
    img = np.empty((8, 8), dtype=np.uint8)
    img[:, :3] = 1
    img[:, 3] = 9
    img[:, 4:] = 2
    img[1, 1] = img[1, 2] = 0
    img[6, 6] = 255
    tree, stats, sums = sh.expected(img, [(1, 1), (1, 6), (1, 2)])
    assert tree[:, 1].tolist() == [mt.ALIVE, mt.ALIVE, 9, 0]
    # record 3: the seed pixel (1, 2) alone, which weighs 0
    assert sums[3].tolist() == [0, 0, 0, 1, 4, 2]
    # record 2 when it died: rows 1 .. 6 of columns 4 .. 6 without (6, 6), all 2s
    rr = 3 * sum(r * r for r in range(1, 7)) - 36
    cc = 6 * (16 + 25 + 36) - 36
    rc = sum(r * c for r in range(1, 7) for c in (4, 5, 6)) - 36
    assert sums[2].tolist() == [2 * rr, 2 * cc, 2 * rc, rr, cc, rc]


# ---- the regimes ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,column", [((8, 70001), 1), ((70001, 8), 0)])
def test_thin_planes_pass_64_bits(shape, column):
    """A weighted sum of 2^64 and more: in columns on the wide plane, in rows on the tall one."""
    r = lc.thin(shape)
    assert lc.accepted(shape[0], shape[1], 65535)
    assert (r.sums[:, column] >= 1 << 64).any(), "no record reaches 2^64"
    assert (r.sums[:, 1 - column] < 1 << 64).all()


def test_three_seas_carry_only_when_the_children_are_joined():
    r = lc.small("three_seas")
    assert lc.accepted(5, 70001, 65535)
    assert r.tree[:, :2].tolist() == [[0, mt.ALIVE], [0, mt.ALIVE], [1, 50], [1, 60]]
    own = r.sums[1] - r.sums[2] - r.sums[3]          # (the two derivations agree on this case: test_two_derivations_agree)
    assert own[1] > 0 and all(x[1] < 1 << 64 for x in (own, r.sums[2], r.sums[3], own + r.sums[2]))
    assert r.sums[1][1] >= 1 << 64


def test_low_word_wraps_more_than_once_on_the_closed_form_plane():
    """3 x (2^24 + 300), every weight 255: the sum of v col^2 is near 2^80, its high word 2^16 -- and its B limb, the sum of the
    terms >> 32, stays below 2^64 as the 2^96 bound promises."""
    h, w = lc.LINE
    assert lc.accepted(h, w, 255)
    sums = sh.closed_form_line_plane(h, w, 255)
    assert sums[1] >> 64 > 1 and sums[1] < 1 << 96
    assert 255 * (w - 1) ** 2 >= 1 << 32          # a single term has a B limb
    assert (w - 1) ** 2 >> 32 > 0                 # and so has a plain one: the plane is not FLAT
    brute = sh.sums_by_key(np.zeros(3 * 1000, dtype=np.int64), sh.terms(np.full((3, 1000), 255)), np.arange(3000), 1)[0]
    assert brute.tolist() == sh.closed_form_line_plane(3, 1000, 255)


def test_a_single_term_of_an_accepted_plane_stays_below_64_bits():
    """A term of 2^64 and more cannot reach the kernels: v row^2 <= wmax * longest^2 <= wmax * pixels * longest, which the stats
    call keeps below 2^64 (check_lake_weights).  The plane the term would need -- a side of 2^24 + 300 under u16 weights -- is
    refused, whatever its other side; the arrival form is run on it with u8 weights instead (test_gpu_lake_shapes)."""
    h, w = lc.LINE
    assert 65535 * (w - 1) ** 2 >= 1 << 64
    assert not lc.accepted(h, w, 65535) and not lc.accepted(1, w, 65535)
    for ph, pw, wmax in ((3, (1 << 24) + 300, 255), (8, 70001, 65535), (1 << 16, 1 << 16, 255)):
        if lc.accepted(ph, pw, wmax):
            assert wmax * (max(ph, pw) - 1) ** 2 < 1 << 64
            assert wmax * ph * pw * max(ph, pw) ** 2 < 1 << 96          # every sum: the header's derivation


def test_small_cases_reach_their_regimes():
    walls = lc.small("walls")
    assert (walls.death[1:] == 0).any(), "no level-0 death"
    assert walls.tree[0, 2] > 0 and any(walls.sums[0]), "record 0 is empty"
    dup = lc.small("duplicates")
    assert (~dup.ex[1:]).any(), "every colour exists"
    assert (lc.small("staircase").death[1:] != mt.ALIVE).sum() >= 254


def test_overflow_case_has_more_roots_in_a_step_than_the_table_has_slots():
    """Nothing floods, so a pixel's root is its own colour for ever (0 for the pixels between the seeds): a workgroup's step of
    1024 consecutive pixels meets 513 distinct roots, more than SHAPE_SLOTS however the probes fall."""
    r = lc.small("overflow")
    assert (r.death[1:] == mt.ALIVE).all() and (r.tree[1:, 2] == 1).all()
    owner = np.zeros(r.img.size, dtype=np.int64)
    owner[r.ps[:, 0] * r.img.shape[1] + r.ps[:, 1]] = np.arange(1, len(r.ps) + 1)
    for step in owner.reshape(-1, 1024):
        assert len(np.unique(step)) == 513 > lc.table_slots()
    assert lc.table_slots() * 100 + 8 <= 64 * 1024          # twelve limbs and a key a slot: what a workgroup may declare


# ---- ellipses -----------------------------------------------------------------------------------------------------------------------

def _records(pkg, pixels, weights):
    """(stats, shapes, area) records of one lake given as (row, col) pixels with integer weights."""
    import lake_stats_ref as ls
    st = ls.empty_records(1)
    st["sum_w"], st["sum_wr"], st["sum_wc"] = sum(weights), sum(v * r for (r, _), v in zip(pixels, weights)), sum(v * c for (_, c), v in zip(pixels, weights))
    st["sum_r"], st["sum_c"] = sum(r for r, _ in pixels), sum(c for _, c in pixels)
    sums = [sum(v * r * r for (r, _), v in zip(pixels, weights)), sum(v * c * c for (_, c), v in zip(pixels, weights)),
            sum(v * r * c for (r, c), v in zip(pixels, weights)), sum(r * r for r, _ in pixels), sum(c * c for _, c in pixels),
            sum(r * c for r, c in pixels)]
    return st, sh.to_words([sums]).view(pkg.api.LAKE_SHAPE_DTYPE), np.array([len(pixels)])


def test_ellipses_hand_cases(pkg):
    E = pkg.ellipses
    st, shp, area = _records(pkg, [(5, 7)], [9])
    assert [float(x[0]) for x in E(st, shp)] == [0.0] * 6
    w = 11
    st, shp, area = _records(pkg, [(4, c) for c in range(3, 3 + w)], [6] * w)
    for got in (E(st, shp), E(st, shp, weighted=False, area=area)):
        var_r, var_c, cov, major, minor, angle = (float(x[0]) for x in got)
        assert (var_r, var_c, cov) == (0.0, (w * w - 1) / 12, 0.0)
        assert major == math.sqrt((w * w - 1) / 12) and minor == 0.0 and angle == math.pi / 2
    st, shp, area = _records(pkg, [(r, 4) for r in range(3, 3 + w)], [6] * w)
    var_r, var_c, cov, major, minor, angle = (float(x[0]) for x in E(st, shp))
    assert (var_r, var_c, cov, angle) == ((w * w - 1) / 12, 0.0, 0.0, 0.0)
    st, shp, area = _records(pkg, [(k, k) for k in range(2, 2 + w)], [1] * w)
    var_r, var_c, cov, major, minor, angle = (float(x[0]) for x in E(st, shp))
    assert var_r == var_c == cov == (w * w - 1) / 12 and angle == math.pi / 4 and minor == 0.0
    st, shp, area = _records(pkg, [(1, 1), (2, 5)], [0, 0])
    assert all(np.isnan(x[0]) for x in E(st, shp))
    assert not any(np.isnan(x[0]) for x in E(st, shp, weighted=False, area=area))
    with pytest.raises(ValueError):
        E(st, shp, weighted=False)


def test_ellipses_are_correctly_rounded_and_agree_with_eigvalsh(pkg):
    r = lc.small("field:96:96:3:1:u16")
    shapes = sh.to_words(r.sums).view(pkg.api.LAKE_SHAPE_DTYPE)
    for weighted in (True, False):
        var_r, var_c, cov, major, minor, angle = pkg.ellipses(r.stats, shapes, weighted=weighted, area=r.tree[:, 2])
        s0 = r.stats["sum_w"] if weighted else r.tree[:, 2]
        s_r, s_c = (r.stats["sum_wr"], r.stats["sum_wc"]) if weighted else (r.stats["sum_r"], r.stats["sum_c"])
        j = 0 if weighted else 3
        seen = 0
        for i in range(len(shapes)):
            S = int(s0[i])
            if S == 0:
                assert np.isnan(var_r[i]) and np.isnan(angle[i]) and np.isnan(major[i]) and np.isnan(minor[i])
                continue
            a = float(Fraction(S * r.sums[i, j] - int(s_r[i]) ** 2, S * S))
            c = float(Fraction(S * r.sums[i, j + 1] - int(s_c[i]) ** 2, S * S))
            b = float(Fraction(S * r.sums[i, j + 2] - int(s_r[i]) * int(s_c[i]), S * S))
            assert (var_r[i], var_c[i], cov[i]) == (a, c, b)
            lo, hi = np.linalg.eigvalsh(np.array([[a, b], [b, c]]))
            tol = 16 * np.finfo(np.float64).eps * max(hi, 0.0)
            assert abs(major[i] ** 2 - hi) <= tol and abs(minor[i] ** 2 - max(lo, 0.0)) <= tol
            assert -math.pi / 2 < angle[i] <= math.pi / 2
            seen += 1
        assert seen > 20
