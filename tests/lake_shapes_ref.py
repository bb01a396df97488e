"""The second moments of ws_merge_tree_shapes in Python integers, following the definition in include/ws_hip.h literally over the
CPU oracle's per-level planes (merge_tree_ref.oracle_planes): record c holds the six sums -- v row^2, v col^2, v row col, row^2,
col^2, row col -- over the pixels equal to c in the plane before c's death level (the last plane if c never died, the seed pixel
alone if it died at level 0: lake_stats_ref.stats_from_planes' selection), record 0 over the pixels the last plane leaves
uncoloured.  Every sum is an unbounded Python int in an object array; `to_words` splits it into the record's (low, high) u64.
`by_folding` is a second derivation: every pixel belongs to the root of its colour at its arrival level, and a record is its own
pixels plus its children's records, folded up `parent` in death order."""
import numpy as np

import lake_stats_ref as ls
import merge_tree_ref as mt

FIELDS = ("sum_wrr", "sum_wcc", "sum_wrc", "sum_rr", "sum_cc", "sum_rc")
DTYPE = np.dtype([(f, "<u8", (2,)) for f in FIELDS])
MASK = (1 << 64) - 1


def terms(v):
    """The six per-pixel terms over the plane v (weights over the padded plane), each a flat object array of Python ints."""
    v = np.asarray(v)
    H, W = v.shape
    r = np.repeat(np.arange(H), W).astype(object)
    c = np.tile(np.arange(W), H).astype(object)
    x = v.ravel().astype(object)
    rr, cc, rc = r * r, c * c, r * c
    return [x * rr, x * cc, x * rc, rr, cc, rc]


def sums_by_key(key, T, idx, n):
    """An (n, 6) object array: row k the six sums over the pixels idx[j] whose key[j] is k; zeros where a key has no pixel."""
    out = np.zeros((n, 6), dtype=object)
    key = np.asarray(key).astype(np.int64)
    if key.size == 0:
        return out
    order = np.argsort(key, kind="stable")
    k = key[order]
    first = np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1])))
    at = k[first]
    pick = np.asarray(idx)[order]
    for j in range(6):
        out[at, j] = np.add.reduceat(T[j][pick], first)
    return out


def sums_of(plane, T, colours):
    """Row i: the six sums over the pixels of `plane` that equal colours[i] (ascending)."""
    colours = np.asarray(colours, dtype=np.int64)
    flat = np.asarray(plane).ravel().astype(np.int64)
    idx = np.flatnonzero(np.isin(flat, colours))
    return sums_by_key(np.searchsorted(colours, flat[idx]), T, idx, len(colours))


def pixel_sums(T, W, r, c):
    return np.array([T[j][r * W + c] for j in range(6)], dtype=object)


def shapes_from_planes(planes, ps, v, death, ex):
    """The (n_seeds + 1, 6) sums from the planes P_0 .. P_max, the seeds in plane coordinates, the weights over the padded plane
    and the death levels and existence flags of merge_tree_ref.tree_from_planes."""
    S = len(ps)
    T = terms(v)
    W = np.asarray(v).shape[1]
    last = len(planes) - 1
    out = np.zeros((S + 1, 6), dtype=object)
    out[0] = sums_of(planes[last], T, [0])[0]
    death = np.asarray(death)
    before = np.where(death == mt.ALIVE, last, death.astype(np.int64) - 1)      # (lake_stats_ref.stats_from_planes' `before`)
    live = np.asarray(ex, dtype=bool).copy()
    live[0] = False
    for L in np.unique(before[live]):
        cols = np.flatnonzero(live & (before == L))
        if L < 0:
            for c in cols:
                out[c] = pixel_sums(T, W, int(ps[c - 1][0]), int(ps[c - 1][1]))
        else:
            out[cols] = sums_of(planes[int(L)], T, cols)
    return out


def by_folding(planes, ps, v, parent, death, ex):
    """The same records another way: own pixels (the plane of a pixel's arrival level names their owner), then children into
    parents in ascending death order; a colour that died at level 0 hands on nothing and takes its seed pixel alone."""
    S = len(ps)
    T = terms(v)
    W = np.asarray(v).shape[1]
    stack = np.stack([np.asarray(p).astype(np.int64) for p in planes])
    shown = stack != 0
    arrival = np.argmax(shown, axis=0)
    owner = np.take_along_axis(stack, arrival[None], axis=0)[0]      # 0 where the pixel never arrives
    out = sums_by_key(owner.ravel(), T, np.arange(owner.size), S + 1)
    death = np.asarray(death)
    dying = np.flatnonzero((death != mt.ALIVE) & np.asarray(ex, dtype=bool))
    for c in dying[np.argsort(death[dying], kind="stable")]:
        if c == 0:
            continue
        if death[c] == 0:
            assert not any(out[c]), "a colour that dies at level 0 owns no pixel"
            out[c] = pixel_sums(T, W, int(ps[c - 1][0]), int(ps[c - 1][1]))
        else:
            out[int(parent[c])] = out[int(parent[c])] + out[c]
    return out


def expected(img, seeds, weights=None, max_level=254, edge=False, seed_shift=False):
    """(tree as an (n_seeds + 1, 4) uint32 array, lake_stats_ref records, (n_seeds + 1, 6) sums) of one call of merge_tree_shapes."""
    planes, ps = mt.oracle_planes(img, seeds, max_level, edge, seed_shift)
    parent, death, area, leaves, vals, ex = mt.tree_from_planes(planes, ps)
    v = ls.plane_weights(img, weights, edge)
    return (np.stack([parent, death, area, leaves], axis=1), ls.stats_from_planes(planes, ps, v, death, ex),
            shapes_from_planes(planes, ps, v, death, ex))


def to_words(sums):
    """(n, 6) Python ints -> records of (low, high) u64 words."""
    sums = np.asarray(sums, dtype=object).reshape(-1, 6)
    rec = np.zeros(len(sums), dtype=DTYPE)
    for j, f in enumerate(FIELDS):
        for i in range(len(sums)):
            x = int(sums[i, j])
            assert 0 <= x < 1 << 128
            rec[f][i] = (x & MASK, x >> 64)
    return rec


def from_words(rec):
    """Records (or the (n, 12) int64 rows DeviceEngine.merge_tree_shapes returns) -> (n, 6) Python ints."""
    w = np.ascontiguousarray(rec).view(np.uint64).reshape(-1, 12)
    return np.array([[int(row[2 * j]) | int(row[2 * j + 1]) << 64 for j in range(6)] for row in w], dtype=object).reshape(-1, 6)


def mismatch(got, want):
    """None, or (records, got, want) where the twelve words of `got` (records or raw rows) differ from the sums `want`."""
    g = np.ascontiguousarray(got).view(np.uint64).reshape(-1, 12)
    w = to_words(want).view(np.uint64).reshape(-1, 12)
    if g.shape != w.shape:
        return "shape", g.shape, w.shape
    bad = np.flatnonzero((g != w).any(axis=1))
    return None if bad.size == 0 else (bad[:6], g[bad[:3]], w[bad[:3]])


def closed_form_line_plane(h, w, v):
    """The six sums of the whole h x w plane with every weight v: sum r^2 = w * sum_{r<h} r^2 and so on."""
    s1 = lambda n: n * (n - 1) // 2
    s2 = lambda n: (n - 1) * n * (2 * n - 1) // 6
    rr, cc, rc = w * s2(h), h * s2(w), s1(h) * s1(w)
    return [v * rr, v * cc, v * rc, rr, cc, rc]
