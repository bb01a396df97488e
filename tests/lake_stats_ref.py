"""The lake statistics of ws_merge_tree_stats derived with numpy from the CPU oracle's per-level planes, following the definition
in include/ws_hip.h literally: record c is measured over the pixels equal to c in the plane before c's death level (the last
plane if c never died, the seed pixel alone if it died at level 0), record 0 over the pixels the last plane leaves uncoloured.
Everything is accumulated in uint64 / int64: what tests/test_gpu_lake_stats.py compares the engine's records against."""
import numpy as np

import merge_tree_ref as mt

NONE = 0xFFFFFFFF
DTYPE = np.dtype([("sum_w", "<u8"), ("sum_wr", "<u8"), ("sum_wc", "<u8"), ("sum_r", "<u8"), ("sum_c", "<u8"),
                  ("r_min", "<u4"), ("r_max", "<u4"), ("c_min", "<u4"), ("c_max", "<u4"), ("w_min", "<u4"), ("w_max", "<u4"),
                  ("peak_pixel", "<u4"), ("reserved", "<u4")])
FIELDS = [n for n in DTYPE.names]


def empty_records(n):
    """n records of the fold's identity: what a colour that does not exist gets."""
    rec = np.zeros(n, dtype=DTYPE)
    for f in ("r_min", "c_min", "w_min", "peak_pixel"):
        rec[f] = NONE
    return rec


def plane_weights(img, weights=None, edge=False):
    """v(p) over the padded plane as int64: the weight plane (None: the image), with edge correction inside a ring of zeros."""
    src = np.asarray(img if weights is None else weights)
    assert src.shape == np.asarray(img).shape
    if not edge:
        return src.astype(np.int64)
    v = np.zeros((src.shape[0] + 2, src.shape[1] + 2), dtype=np.int64)
    v[1:-1, 1:-1] = src
    return v


def records_by_key(key, val, idx, W, n):
    """Record k (0 <= k < n) over the pixels listed: pixel j has key key[j], weight val[j] and row-major index idx[j] (ascending)
    in a plane W wide; the identity where a key has no pixel.  Exact: a stable sort by key, then integer reductions per run."""
    key = np.asarray(key).astype(np.int64)
    rec = empty_records(n)
    if key.size == 0:
        return rec
    order = np.argsort(key, kind="stable")          # within a key the pixels stay in row-major order
    k = key[order]
    val = np.asarray(val).astype(np.uint64)[order]
    idx = np.asarray(idx).astype(np.uint64)[order]
    first = np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1])))
    at = k[first]
    row, col = idx // np.uint64(W), idx % np.uint64(W)
    rec["sum_w"][at] = np.add.reduceat(val, first)
    rec["sum_wr"][at] = np.add.reduceat(val * row, first)
    rec["sum_wc"][at] = np.add.reduceat(val * col, first)
    rec["sum_r"][at] = np.add.reduceat(row, first)
    rec["sum_c"][at] = np.add.reduceat(col, first)
    rec["r_min"][at] = np.minimum.reduceat(row, first)
    rec["r_max"][at] = np.maximum.reduceat(row, first)
    rec["c_min"][at] = np.minimum.reduceat(col, first)
    rec["c_max"][at] = np.maximum.reduceat(col, first)
    rec["w_min"][at] = np.minimum.reduceat(val, first)
    top = np.maximum.reduceat(val, first)
    rec["w_max"][at] = top
    run = np.cumsum(np.concatenate(([True], k[1:] != k[:-1]))) - 1
    # the FIRST pixel in row-major order that holds the run's largest weight
    rec["peak_pixel"][at] = np.minimum.reduceat(np.where(val == top[run], idx, np.uint64(NONE)), first)
    return rec


def records_by_label(plane, v, n):
    """Record l (0 <= l < n) over the pixels of `plane` that equal l; the identity where there is none."""
    plane = np.asarray(plane)
    return records_by_key(plane.ravel(), np.asarray(v).ravel(), np.arange(plane.size), plane.shape[1], n)


def pixel_record(v, r, c):
    """The record of the single pixel (r, c)."""
    W = np.asarray(v).shape[1]
    x = int(np.asarray(v)[r, c])
    rec = empty_records(1)
    rec[0] = (x, x * r, x * c, r, c, r, r, c, c, x, x, r * W + c, 0)
    return rec[0]


def stats_from_planes(planes, ps, v, death, ex):
    """The n_seeds + 1 records from the planes P_0 .. P_max, the seeds in plane coordinates, the weights over the padded plane and
    the death levels and existence flags of merge_tree_ref.tree_from_planes."""
    S = len(ps)
    rec = empty_records(S + 1)
    by_level = {}

    def level(L):
        if L not in by_level:
            by_level[L] = records_by_label(planes[L], v, S + 1)
        return by_level[L]

    rec[0] = level(len(planes) - 1)[0]
    for c in range(1, S + 1):
        if not ex[c]:
            continue
        before = int(death[c]) - 1 if death[c] != mt.ALIVE else len(planes) - 1
        rec[c] = pixel_record(v, int(ps[c - 1][0]), int(ps[c - 1][1])) if before < 0 else level(before)[c]
    return rec


def expected(img, seeds, weights=None, max_level=254, edge=False, seed_shift=False):
    """(tree as an (n_seeds + 1, 4) uint32 array, stats) for one call of merge_tree_stats."""
    planes, ps = mt.oracle_planes(img, seeds, max_level, edge, seed_shift)
    parent, death, area, leaves, vals, ex = mt.tree_from_planes(planes, ps)
    rec = stats_from_planes(planes, ps, plane_weights(img, weights, edge), death, ex)
    return np.stack([parent, death, area, leaves], axis=1), rec


def join(records):
    """The fold of a set of records into one (the identity for none)."""
    out = empty_records(1)[0]
    records = np.asarray(records, dtype=DTYPE)
    if records.size == 0:
        return out
    for f in ("sum_w", "sum_wr", "sum_wc", "sum_r", "sum_c"):
        out[f] = records[f].sum(dtype=np.uint64)
    for f in ("r_min", "c_min", "w_min"):
        out[f] = records[f].min()
    for f in ("r_max", "c_max", "w_max"):
        out[f] = records[f].max()
    top = records[(records["w_max"] == out["w_max"]) & (records["peak_pixel"] != NONE)]
    out["peak_pixel"] = top["peak_pixel"].min() if top.size else NONE
    return out


def join_pairwise(a, b):
    """Element by element, the fold of record a[i] with record b[i]."""
    out = np.empty(a.shape, dtype=DTYPE)
    for f in ("sum_w", "sum_wr", "sum_wc", "sum_r", "sum_c"):
        out[f] = a[f] + b[f]
    for f in ("r_min", "c_min", "w_min"):
        out[f] = np.minimum(a[f], b[f])
    for f in ("r_max", "c_max", "w_max"):
        out[f] = np.maximum(a[f], b[f])
    # the larger weight wins the peak, the earlier pixel a tie (an empty side has weight 0 and pixel NONE: it never wins a tie)
    take_b = (b["w_max"] > a["w_max"]) | ((b["w_max"] == a["w_max"]) & (b["peak_pixel"] < a["peak_pixel"]))
    out["peak_pixel"] = np.where(take_b, b["peak_pixel"], a["peak_pixel"])
    out["reserved"] = 0
    return out


def join_by_key(key, records, n):
    """Record k (0 <= k < n): the fold of the records whose key is k; the identity where there is none."""
    key = np.asarray(key).astype(np.int64)
    out = empty_records(n)
    if key.size == 0:
        return out
    order = np.argsort(key, kind="stable")
    k, r = key[order], records[order]
    first = np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1])))
    at = k[first]
    run = np.cumsum(np.concatenate(([True], k[1:] != k[:-1]))) - 1
    for f in ("sum_w", "sum_wr", "sum_wc", "sum_r", "sum_c"):
        out[f][at] = np.add.reduceat(np.ascontiguousarray(r[f]), first)
    for f in ("r_min", "c_min", "w_min"):
        out[f][at] = np.minimum.reduceat(np.ascontiguousarray(r[f]), first)
    for f in ("r_max", "c_max", "w_max"):
        out[f][at] = np.maximum.reduceat(np.ascontiguousarray(r[f]), first)
    top = out["w_max"][at]
    out["peak_pixel"][at] = np.minimum.reduceat(np.where(r["w_max"] == top[run], r["peak_pixel"], np.uint32(NONE)), first)
    return out


def from_raw(raw):
    """The (n, 9) int64 rows DeviceEngine.merge_tree_stats returns, as records."""
    return np.ascontiguousarray(raw).view(DTYPE).reshape(-1)


def mismatch(got, want):
    """None, or (field, indices, got, want) of the first field that differs."""
    for f in FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        if bad.size:
            return f, bad[:8], got[f][bad[:8]], want[f][bad[:8]]
    return None
