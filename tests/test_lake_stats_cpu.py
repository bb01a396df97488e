"""merge_tree_stats without a GPU: the record's layout and the new symbols at the boundary, and the numpy derivation of the
records from the CPU oracle's planes (tests/lake_stats_ref.py) on a hand-made case whose records are written out here.  The
refusals that need a context to report through are in tests/test_gpu_lake_stats.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import lake_stats_ref as ls
import merge_tree_ref as mt
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ws_merge_tree_stats_device", "ws_merge_tree_stats")
N = ls.NONE


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


def test_record_is_72_bytes_with_the_headers_offsets(pkg):
    S = pkg._ffi.LakeStats
    assert ctypes.sizeof(S) == 72
    want = [("sum_w", 0), ("sum_wr", 8), ("sum_wc", 16), ("sum_r", 24), ("sum_c", 32), ("r_min", 40), ("r_max", 44), ("c_min", 48),
            ("c_max", 52), ("w_min", 56), ("w_max", 60), ("peak_pixel", 64), ("reserved", 68)]
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == want
    for dtype in (pkg.api.LAKE_STATS_DTYPE, ls.DTYPE):
        assert dtype.itemsize == 72
        assert [(f, dtype.fields[f][1]) for f in dtype.names] == want


def test_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "ws_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(pkg._ffi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in pkg._ffi.SIGNATURES
        assert getattr(raw, name) is not None
    assert "typedef struct ws_lake_stats" in code
    assert pkg._ffi.lib().ws_abi_version() == pkg._ffi.WS_ABI_VERSION == 3


def test_new_names_in_every_mirror(pkg):
    ffi_rs = open(os.path.join(ROOT, "rust", "src", "hip_ffi.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert re.search(r"\bfn\s+" + name + r"\s*\(", ffi_rs), name
        assert re.search(r"\bfn\s+" + name + r"\s*\(", doc), name
    assert "pub struct ws_lake_stats" in ffi_rs
    assert "merge_tree_stats" in open(os.path.join(ROOT, "include", "ws_watershed.hpp")).read()
    assert "merge_tree_stats" in open(os.path.join(ROOT, "rust", "src", "watershed_hip.rs")).read()
    assert hasattr(pkg.MergingWatershed, "merge_tree_stats") and not hasattr(pkg.SegmentingWatershed, "merge_tree_stats")
    assert callable(pkg.centroids)


def test_null_context_is_bad_arg(pkg):
    L = pkg._ffi.lib()
    opt = pkg._ffi.Options()
    img = np.zeros((4, 4), dtype=np.uint8)
    seeds = np.zeros((1, 2), dtype=np.uint64)
    tree = np.zeros((2, 4), dtype=np.uint32)
    stats = np.zeros(2, dtype=ls.DTYPE)
    for name in NEW:
        rc = getattr(L, name)(None, img.ctypes.data, 4, 4, 4, seeds.ctypes.data, 1, ctypes.byref(opt), None, 0, 0, tree.ctypes.data,
                              stats.ctypes.data, None)
        assert rc == pkg._ffi.WS_ERR_BAD_ARG, name


def _hand_made():
    """8 x 8 (its border never floods: lib.rs floods interior pixels only): a basin of 1s (columns 1, 2) and a basin of 2s (columns
    4 .. 6) either side of a ridge of 9s in column 3.  Seeds: colour 1 at (1, 1) and colour 3 at (1, 2), both on a 0 -- they touch
    at level 0, so 3 dies there into 1 -- and colour 2 at (1, 6).  Pixel (6, 6) is 255 and never floods.  The basins meet when the
    ridge floods: 2 dies at level 9 into 1."""
    img = np.empty((8, 8), dtype=np.uint8)
    img[:, :3] = 1
    img[:, 3] = 9
    img[:, 4:] = 2
    img[1, 1] = img[1, 2] = 0
    img[6, 6] = 255
    return img, [(1, 1), (1, 6), (1, 2)]


def test_reference_on_a_hand_made_case():
    img, seeds = _hand_made()
    tree, rec = ls.expected(img, seeds)
    A = mt.ALIVE
    assert tree.tolist() == [[0, A, 29, 0], [0, A, 35, 3], [1, 9, 17, 1], [1, 0, 1, 1]]
    want = [
        # record 0: the 28 border pixels and (6, 6).  Top and bottom row weigh 3 * 1 + 9 + 4 * 2 = 20 each, their weighted
        # columns 1 * (0 + 1 + 2) + 9 * 3 + 2 * (4 + 5 + 6 + 7) = 74; the left side (rows 1 .. 6) weighs 6, the right 12
        (20 + 20 + 6 + 12 + 255, 20 * 7 + 1 * 21 + 2 * 21 + 255 * 6, 74 + 74 + 2 * 7 * 6 + 255 * 6, 8 * 7 + 2 * 21 + 6,
         28 + 28 + 7 * 6 + 6, 0, 7, 0, 7, 1, 255, 6 * 8 + 6, 0),
        # record 1, the survivor: the 6 x 6 interior without (6, 6): ten 1s (rows 2 .. 6 of columns 1, 2), the ridge, the 2s
        (10 + 6 * 9 + 17 * 2, 2 * 20 + 9 * 21 + 114, 5 * 3 + 9 * 3 * 6 + 168, 6 * 21 - 6, 6 * 21 - 6, 1, 6, 1, 6, 0, 9, 1 * 8 + 3, 0),
        # record 2 when it died: rows 1 .. 6 of columns 4 .. 6 without (6, 6), all 2s
        (17 * 2, 2 * (3 * 21 - 6), 2 * (6 * 15 - 6), 3 * 21 - 6, 6 * 15 - 6, 1, 6, 4, 6, 2, 2, 1 * 8 + 4, 0),
        # record 3 died at level 0: its seed pixel alone, a 0 at (1, 2)
        (0, 0, 0, 1, 2, 1, 1, 2, 2, 0, 0, 1 * 8 + 2, 0)]
    assert [tuple(int(x) for x in r) for r in rec] == want


def test_reference_with_weights_and_edge_correction_on_the_hand_made_case():
    """The same image under edge correction (seed_shift keeps the seeds on their pixels; now the image's border floods and the
    ring of the padded plane does not), weighed by a u16 plane that is 1000 everywhere but 65535 at (2, 5) and (6, 5) and 0 at
    (0, 6)."""
    img, seeds = _hand_made()
    wt = np.full((8, 8), 1000, dtype=np.uint16)
    wt[2, 5] = wt[6, 5] = 65535
    wt[0, 6] = 0
    tree, rec = ls.expected(img, seeds, weights=wt, edge=True, seed_shift=True)
    v = ls.plane_weights(img, wt, edge=True)
    assert v.shape == (10, 10) and v[0].sum() == 0 and v[:, 9].sum() == 0 and v[3, 6] == 65535 and v[1, 7] == 0
    # colour 2 holds the 2s when it dies: padded rows 1 .. 8, columns 5 .. 8 without (7, 7)
    assert tree[2].tolist() == [1, 9, 31, 1]
    r = rec[2]
    assert (int(r["r_min"]), int(r["r_max"]), int(r["c_min"]), int(r["c_max"])) == (1, 8, 5, 8)
    assert int(r["sum_w"]) == 28 * 1000 + 2 * 65535 and int(r["w_min"]) == 0 and int(r["w_max"]) == 65535
    assert int(r["peak_pixel"]) == 3 * 10 + 6          # the first of the two 65535s
    assert int(r["sum_wr"]) == 65535 * (3 + 7) + 1000 * (4 * 36 - 7 - 3 - 7 - 1)
    # record 3: its seed pixel alone, (1, 2) of the image at (2, 3) of the padded plane
    assert tuple(int(x) for x in rec[3]) == (1000, 2000, 3000, 2, 3, 2, 2, 3, 3, 1000, 1000, 23, 0)
    # uncoloured: the ring, which weighs nothing, and (7, 7)
    assert tree[0].tolist() == [0, mt.ALIVE, 37, 0]
    assert tuple(int(x) for x in rec[0]) == (1000, 7000, 7000, 2 * 90 - 2 * 9 + 7, 2 * 90 - 2 * 9 + 7, 0, 9, 0, 9, 0, 1000, 77, 0)


def test_reference_records_join_to_the_plane(pkg):
    img = cases.field(50, 70, 2)
    seeds = ol.find_local_minima(img)
    tree, rec = ls.expected(img, seeds)
    alive = (tree[:, 1] == mt.ALIVE) & (tree[:, 3] > 0)
    alive[0] = True
    whole = ls.records_by_label(np.zeros(img.shape, dtype=np.int64), img, 1)[0]
    assert ls.join(rec[alive]) == whole
    gone = tree[:, 3] == 0
    gone[0] = False
    assert (rec[gone] == ls.empty_records(1)[0]).all()
    row, col = pkg.centroids(rec)
    has = rec["sum_w"] > 0
    assert np.isnan(row[~has]).all() and np.isnan(col[~has]).all()
    assert ((row[has] >= rec["r_min"][has]) & (row[has] <= rec["r_max"][has])).all()
    assert ((col[has] >= rec["c_min"][has]) & (col[has] <= rec["c_max"][has])).all()
