"""Thin planes and huge cubes: inputs with a side past 2^16 (tier A), past 2^24 (tier B) and a cube of more than 2^16 slices (tier C),
in plain numpy, with what the CPU oracle says about each.  tests/test_extreme_cases_cpu.py proves without a GPU that the inputs and
the expected values are what they claim, tests/test_gpu_extreme_shapes.py compares the engine with them bit for bit.

Tier A: the oracle runs on the plane itself (`products`).  Tier B: the plane is a chain of PIECES of P = 1021 lines along its long
axis, each a cases.field whose first and last line are walls (255 is never flooded, so every piece floods alone); the pieces come
from N_PATTERNS patterns in the order (3 i^2 + i) % N_PATTERNS and a shorter remainder piece closes the plane.  The oracle runs
once per pattern and the expected plane is the patterns' results laid end to end, colours offset into the whole list's numbering
(`Chain`).  2^24 % P = 144, so a row index that wraps at 24 bits lands on another phase of another pattern, and P is prime, so the
pieces meet the 64-, 128- and 256-line tile grids at every phase.  Tier C: 70001 slices of 8 x 16 drawn from 17 distinct slices in
the order (3 i^2 + i) % 17, values below 16 and max_water_level 15, so that the list products stay near 7 M records (`Cube`).

`products` derives every per-level product from ONE run of each oracle while it runs -- no plane but the last is kept, no Python
loop over colours -- following the definitions of merge_tree_ref and lake_stats_ref; the CPU test proves it equal to those two."""
import numpy as np

import cases
import lake_stats_ref as ls
import merge_tree_ref as mt
import oracle_lib as ol

KEY_INF = 0xFF000000
P = 1021
N_PATTERNS = 7
N_DISTINCT = 17

TIER_A_TALL = [(70001, 8), (262153, 5), (70001, 3), (70001, 2), (70001, 1)]
TIER_A = TIER_A_TALL + [(w, h) for h, w in TIER_A_TALL]
TIER_A_LEVELS = [0, 127, 254]
TIER_B = [((1 << 24) + 70, 4), ((1 << 24) + 70, 3), (4, (1 << 24) + 72), (3, (1 << 24) + 70)]
TIER_B_LEVELS = [0, 254]
TIER_C = (70001, 8, 16)
TIER_C_MAX_LEVEL = 15
TIER_C_LEVELS = [0, 7, 15]


def order(n, m):
    """Which of m patterns piece (slice) i = 0 .. n - 1 is: (3 i^2 + i) % m.  (A quadratic residue order: with m prime it reaches
    (m + 1) / 2 of the patterns -- 4 of 7, 9 of 17 -- in a sequence whose neighbours differ.)"""
    i = np.arange(n, dtype=np.int64)
    return (3 * i * i + i) % m


def pack_stamps(keys64):
    """The oracle's stamps (level << 32 | ring, ~0 for "never") in the engine's form (level << 24 | ring, KEY_INF for "never")."""
    never = keys64 == np.uint64(0xFFFFFFFFFFFFFFFF)
    packed = ((keys64 >> np.uint64(32)) << np.uint64(24)) | (keys64 & np.uint64(0xFFFFFF))
    return np.where(never, np.uint64(KEY_INF), packed).astype(np.uint32)


def stamps_mismatch(got, want):
    """None, or where an engine's stamp plane differs from pack_stamps' ("never" is any stamp from KEY_INF up)."""
    got = np.minimum(np.asarray(got).view(np.uint32), np.uint32(KEY_INF))
    bad = np.flatnonzero(got.ravel() != want.ravel())
    return None if bad.size == 0 else (bad.size, bad[:6], got.ravel()[bad[:6]], want.ravel()[bad[:6]])


def weights_u16(shape, seed):
    """A u16 weight plane that holds 0 and 65535 many times (ties for w_min, w_max and the peak pixel)."""
    rng = np.random.default_rng(7000 + seed)
    w = rng.integers(0, 65536, shape, dtype=np.uint16)
    w[rng.random(shape) < 0.02] = 65535
    w[rng.random(shape) < 0.02] = 0
    return w


# ---- every product of one plane from one run of each oracle -------------------------------------------------------------------------

class Products:
    """labels, stamps: the segmenting transform's labels (u32) and packed stamps.  final: the merging transform's last plane (u32).
    planes, seg_planes: level -> merging / segmenting plane (u32) for the levels asked for.  lakes, seg_lakes: per level
    (colours ascending, their areas, uncoloured pixels).  tree: (S + 1, 4) u32 parent, death, area, leaves.  stats: lake_stats_ref
    records under the weight plane given (None where none was)."""
    __slots__ = ("ps", "labels", "stamps", "final", "planes", "seg_planes", "lakes", "seg_lakes", "tree", "stats", "max_rings")


def _pixel_records(v, rows, cols):
    """lake_stats_ref.pixel_record of many single pixels at once."""
    W = v.shape[1]
    x = v[rows, cols].astype(np.uint64)
    r, c = rows.astype(np.uint64), cols.astype(np.uint64)
    rec = ls.empty_records(len(rows))
    rec["sum_w"], rec["sum_wr"], rec["sum_wc"], rec["sum_r"], rec["sum_c"] = x, x * r, x * c, r, c
    rec["r_min"] = rec["r_max"] = r
    rec["c_min"] = rec["c_max"] = c
    rec["w_min"] = rec["w_max"] = x
    rec["peak_pixel"] = r * np.uint64(W) + c
    return rec


def _records_of(plane, v, colours):
    """lake_stats_ref records of the (ascending) colours given, over the pixels of `plane` that carry one of them."""
    pick = np.zeros(int(colours[-1]) + 1 if len(colours) else 1, dtype=bool)
    pick[colours] = True
    flat = plane.ravel()
    idx = np.flatnonzero(pick[np.minimum(flat, len(pick) - 1)] & (flat < len(pick)))
    return ls.records_by_key(np.searchsorted(colours, flat[idx]), v.ravel()[idx], idx, plane.shape[1], len(colours))


def products(img, seeds, max_level=254, edge=False, levels=(), weights=None, want_lists=True):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    ps = np.asarray(seeds, dtype=np.int64).reshape(-1, 2)
    S = len(ps)
    out = Products()
    out.ps = ps
    labels64, keys64 = ol.segment_arrival(img, ps, max_level=max_level, edge=edge, want_keys=True)
    out.labels = labels64.astype(np.uint32)
    out.stamps = pack_stamps(keys64)
    coloured = out.stamps != KEY_INF
    out.max_rings = int((out.stamps[coloured] & np.uint32(0xFFFFFF)).max()) if coloured.any() else 0
    del labels64, keys64
    # the segmenting transform's planes and lists: a pixel is coloured from its arrival level on and keeps its colour
    arrived = np.where(coloured, out.stamps >> np.uint32(24), np.uint32(255)).ravel()
    out.seg_planes = {L: np.where((arrived <= L).reshape(out.labels.shape), out.labels, np.uint32(0)) for L in levels}
    out.seg_lakes = []
    if want_lists:
        by_level = np.argsort(arrived, kind="stable")
        first = np.searchsorted(arrived[by_level], np.arange(max_level + 2))
        flat = out.labels.ravel()
        cur = np.zeros(S + 1, dtype=np.int64)
        for L in range(max_level + 1):
            cur += np.bincount(flat[by_level[first[L]:first[L + 1]]], minlength=S + 1)
            cols = np.flatnonzero(cur[1:]) + 1
            out.seg_lakes.append((cols, cur[cols].copy(), int(flat.size - first[L + 1])))
        del by_level
    # the merging transform: every level's canonical plane as the oracle hands it over, folded at once
    ex = np.zeros(S + 1, dtype=bool)
    if S:
        if len(np.unique(ps[:, 0] * out.labels.shape[1] + ps[:, 1])) == S:
            ex[1:] = True
        else:                                       # duplicates: the later entry wins, in list order
            ex[:] = mt.existing(ps, out.labels.shape)
    v = None if weights is None else ls.plane_weights(img, weights, edge)
    parent = np.zeros(S + 1, dtype=np.uint32)
    death = np.full(S + 1, mt.ALIVE, dtype=np.uint32)
    area = np.zeros(S + 1, dtype=np.uint32)
    leaves = np.zeros(S + 1, dtype=np.uint32)
    stats = ls.empty_records(S + 1) if v is not None else None
    alive = ex.copy()
    alive[0] = False
    colour = np.arange(S + 1, dtype=np.int64)
    st = {"plane": None, "hist": None, "leaf": None, "n": 0}
    out.planes, out.lakes = {}, []
    want = set(int(L) for L in levels)

    def level(L, _mx, _img, plane):
        L = int(L)
        assert L == st["n"]
        st["n"] += 1
        cur = plane.astype(np.uint32)
        hist = np.bincount(cur.ravel(), minlength=S + 1)
        vals = np.zeros(S + 1, dtype=np.int64)
        if S:
            vals[1:] = cur[ps[:, 0], ps[:, 1]]
        leaf = np.bincount(vals[ex], minlength=S + 1)
        dying = np.flatnonzero(alive & (vals != colour))
        if dying.size:
            death[dying], parent[dying] = L, vals[dying]
            alive[dying] = False
            if L == 0:
                area[dying] = leaves[dying] = 1
                if v is not None:
                    stats[dying] = _pixel_records(v, ps[dying - 1, 0], ps[dying - 1, 1])
            else:
                area[dying], leaves[dying] = st["hist"][dying], st["leaf"][dying]
                if v is not None:
                    stats[dying] = _records_of(st["plane"], v, dying)
        if want_lists:
            cols = np.flatnonzero(hist[1:]) + 1
            out.lakes.append((cols, hist[cols], int(hist[0])))
        if L in want:
            out.planes[L] = cur
        st["plane"], st["hist"], st["leaf"] = cur, hist, leaf

    final = ol.merge_arrival(img, ps, max_level=max_level, edge=edge, hook=level)
    assert st["n"] == max_level + 1
    out.final = final.astype(np.uint32)
    assert (out.final == st["plane"]).all()
    last = np.flatnonzero(alive)
    area[last], leaves[last] = st["hist"][last], st["leaf"][last]
    area[0] = st["hist"][0]
    if v is not None:
        keep = np.concatenate(([0], last))
        stats[keep] = _records_of(st["plane"], v, keep)
    out.tree = np.stack([parent, death, area, leaves], axis=1)
    out.stats = stats
    return out


# ---- tier A -----------------------------------------------------------------------------------------------------------------------

def tier_a_input(shape):
    """(image, seeds): cases.field with its own maxima as seeds; a plane without an interior gets two hand-placed seeds."""
    h, w = shape
    img = cases.field(h, w, 11 * h + w)
    if min(h, w) >= 3:
        seeds = ol.find_local_minima(img).astype(np.int64)
    elif h >= w:
        seeds = np.array([[h // 3, 0], [h - 2, w - 1]], dtype=np.int64)
    else:
        seeds = np.array([[0, w // 3], [h - 1, w - 2]], dtype=np.int64)
    return img, seeds


# ---- tier B: a chain of pieces --------------------------------------------------------------------------------------------------------

class Chain:
    """The plane of `shape` as pieces of `piece` lines along its long axis.  tall: the pieces are runs of rows; else of columns.
    img, seeds (the whole plane's row-major list), weights (u16), weights8 (their high bytes), and the stitched expected values:
    labels, stamps, final, plane(level), tree, stats."""

    def __init__(self, shape, piece=P, n_patterns=N_PATTERNS, levels=TIER_B_LEVELS, seed=0):
        h, w = shape
        self.shape, self.tall, self.piece = shape, h >= w, piece
        self.long, self.short = max(h, w), min(h, w)
        self.n_full, self.rem = divmod(self.long, piece)
        assert self.rem >= 3
        self.which = order(self.n_full, n_patterns)
        self.levels = list(levels)
        # the patterns (and the remainder as one more), each with walls on its first and last line
        self.pat_img, self.pat_wt, self.pat, self.pat_wt8, self.pat_stats8 = [], [], [], [], []
        for k in range(n_patterns + 1):
            lines = piece if k < n_patterns else self.rem
            f = cases.field(*((lines, self.short) if self.tall else (self.short, lines)), 1000 * seed + 10 * self.short + k)
            if self.tall:
                f[0, :] = 255
                if k < n_patterns:
                    f[-1, :] = 255
            else:
                f[:, 0] = 255
                if k < n_patterns:
                    f[:, -1] = 255
            self.pat_img.append(f)
            self.pat_wt.append(weights_u16(f.shape, 50 * seed + k))
            self.pat.append(products(f, ol.find_local_minima(f).astype(np.int64), levels=self.levels, weights=self.pat_wt[-1], want_lists=False))
            # (the same flood weighed by the u16 plane's high bytes: wmax * pixels * lines of a 2^24-line plane passes 2^64 with
            # u16 weights, which ws_merge_tree_stats refuses -- u8 weights are what reaches its kernels there)
            self.pat_wt8.append((self.pat_wt[-1] >> 8).astype(np.uint8))
            self.pat_stats8.append(products(f, self.pat[-1].ps, weights=self.pat_wt8[-1], want_lists=False).stats)
        self.kind = np.concatenate([self.which, [n_patterns]])            # pattern of every piece, the remainder last
        self.n_seeds_of = np.array([len(p.ps) for p in self.pat], dtype=np.int64)
        self.base = np.concatenate([[0], np.cumsum(self.n_seeds_of[self.kind])])      # piece i's seeds in piece-major order
        self.start = np.arange(len(self.kind), dtype=np.int64) * piece                 # piece i's first line
        self.n_seeds = int(self.base[-1])
        self._colours()
        self.img = self._lay(self.pat_img)
        self.weights = self._lay(self.pat_wt)
        self.weights8 = self._lay(self.pat_wt8)

    def _colours(self):
        """seeds: the whole plane's list in row-major order.  colour[j]: the whole list's colour of piece-major seed j (piece i's
        local colour c is j = base[i] + c - 1).  Tall planes: the piece-major order IS row-major.  Wide planes: a stable sort by
        row interleaves the pieces and keeps every piece's own order."""
        rows = np.empty(self.n_seeds, dtype=np.int64)
        cols = np.empty(self.n_seeds, dtype=np.int64)
        for k, p in enumerate(self.pat):
            at = np.flatnonzero(self.kind == k)
            if p.ps.shape[0] == 0 or at.size == 0:
                continue
            j = (self.base[at][:, None] + np.arange(len(p.ps))[None, :]).ravel()
            off = np.repeat(self.start[at], len(p.ps))
            rows[j] = np.tile(p.ps[:, 0], at.size) + (off if self.tall else 0)
            cols[j] = np.tile(p.ps[:, 1], at.size) + (0 if self.tall else off)
        by = np.argsort(rows, kind="stable") if not self.tall else np.arange(self.n_seeds)
        self.seeds = np.stack([rows[by], cols[by]], axis=1)
        self.colour = np.empty(self.n_seeds + 1, dtype=np.int64)
        self.colour[0] = 0
        self.colour[1 + by] = np.arange(1, self.n_seeds + 1)

    def _lay(self, per_pattern, colours=False):
        """The patterns' planes laid end to end; colours: local colours go through `colour` (0 stays 0)."""
        first = per_pattern[0]
        out = np.empty(self.shape, dtype=np.uint32 if colours else first.dtype)
        body = out[: self.n_full * self.piece] if self.tall else None
        stack = np.empty((self.n_full,) + first.shape, dtype=out.dtype)
        for k, plane in enumerate(per_pattern):
            at = np.flatnonzero(self.kind == k)
            for_pieces = at[at < self.n_full]
            if colours:
                lut = self.base[at][:, None] + np.arange(self.n_seeds_of[k] + 1)[None, :]      # piece-major index + 1 of local colour c
                lut = self.colour[lut]
                lut[:, 0] = 0
                vals = lut[:, plane.astype(np.int64)]          # (pieces, rows, cols)
            else:
                vals = np.broadcast_to(plane, (at.size,) + plane.shape)
            if k < len(per_pattern) - 1:
                stack[for_pieces] = vals
            else:
                tail = vals[0]
        if self.tall:
            body[:] = stack.reshape(self.n_full * self.piece, self.short)
            out[self.n_full * self.piece:] = tail
        else:
            out[:, : self.n_full * self.piece] = stack.transpose(1, 0, 2).reshape(self.short, self.n_full * self.piece)
            out[:, self.n_full * self.piece:] = tail
        return out

    # the stitched expected values, built when asked for (each once)
    def labels(self):
        return self._lay([p.labels for p in self.pat], colours=True)

    def stamps(self):
        return self._lay([p.stamps for p in self.pat])

    def final(self):
        return self._lay([p.final for p in self.pat], colours=True)

    def plane(self, level, merging=True):
        return self._lay([(p.planes if merging else p.seg_planes)[level] for p in self.pat], colours=True)

    def tree(self):
        """Local parents move into the whole list's numbering like the colours; record 0 counts every piece's uncoloured pixels."""
        out = np.zeros((self.n_seeds + 1, 4), dtype=np.uint32)
        for k, p in enumerate(self.pat):
            at = np.flatnonzero(self.kind == k)
            S = len(p.ps)
            if S == 0 or at.size == 0:
                continue
            j = self.base[at][:, None] + np.arange(1, S + 1)[None, :]
            g = self.colour[j]                                                     # (pieces, S)
            par = p.tree[1:, 0].astype(np.int64)
            gp = self.colour[self.base[at][:, None] + np.maximum(par, 1)[None, :]]
            out[g, 0] = np.where(par[None, :] > 0, gp, 0)
            out[g, 1:] = p.tree[1:, 1:][None, :, :]
        out[0] = (0, mt.ALIVE, sum(int(self.pat[k].tree[0, 2]) for k in self.kind), 0)
        return out

    def stats(self, u8=False):
        """Catalogue records (u8: under weights8): a piece's local records moved by its first line -- tall: sum_r += area * row0,
        sum_wr += sum_w * row0, r_min / r_max += row0, peak_pixel += row0 * W; wide: the same in the column fields, the peak
        pixel recomputed from its local (row, column).  Record 0 is the fold of every piece's record 0."""
        W = self.shape[1]
        out = ls.empty_records(self.n_seeds + 1)
        zero_rec = []
        sums = ("sum_r", "sum_wr", "r_min", "r_max") if self.tall else ("sum_c", "sum_wc", "c_min", "c_max")
        for k, p in enumerate(self.pat):
            at = np.flatnonzero(self.kind == k)
            if at.size == 0:
                continue
            S = len(p.ps)
            local = np.tile(self.pat_stats8[k] if u8 else p.stats, at.size).reshape(at.size, S + 1)
            off = self.start[at].astype(np.uint64)[:, None]
            n = np.concatenate(([p.tree[0, 2]], p.tree[1:, 2])).astype(np.uint64)[None, :]      # pixels a record is measured over
            lw = self.pat_img[k].shape[1]
            has = local["peak_pixel"] != ls.NONE
            local[sums[0]] += n * off
            local[sums[1]] += local["sum_w"] * off
            for f in sums[2:]:
                local[f] = np.where(has, local[f] + off.astype(np.uint32), local[f])
            pk = local["peak_pixel"].astype(np.uint64)
            moved = pk + off * np.uint64(W) if self.tall else (pk // np.uint64(lw)) * np.uint64(W) + pk % np.uint64(lw) + off
            local["peak_pixel"] = np.where(has, moved, np.uint64(ls.NONE)).astype(np.uint32)
            if S:
                g = self.colour[self.base[at][:, None] + np.arange(1, S + 1)[None, :]]
                out[g] = local[:, 1:]
            zero_rec.append(local[:, 0])
        zr = np.concatenate(zero_rec)
        out[0] = ls.join_by_key(np.zeros(len(zr), dtype=np.int64), zr, 1)[0]
        return out


# ---- tier C: a cube of many thumbnails ---------------------------------------------------------------------------------------------

class Cube:
    """n slices of h x w from N_DISTINCT distinct slices (values below 16, every one with a seed), in the order (3 i^2 + i) %
    N_DISTINCT; `distinct[k]`: the products of distinct slice k at max_water_level 15."""

    def __init__(self, n=TIER_C[0], h=TIER_C[1], w=TIER_C[2], n_distinct=N_DISTINCT, max_level=TIER_C_MAX_LEVEL, levels=TIER_C_LEVELS):
        self.n, self.h, self.w, self.max_level, self.levels = n, h, w, max_level, list(levels)
        self.which = order(n, n_distinct)
        self.imgs, self.wts, self.distinct = [], [], []
        k = 0
        while len(self.imgs) < n_distinct:
            f = (cases.field(h, w, 400 + k) % 16).astype(np.uint8)
            k += 1
            s = ol.find_local_minima(f).astype(np.int64)
            if len(s) == 0:
                continue
            self.imgs.append(f)
            self.wts.append(weights_u16(f.shape, 900 + k))
            self.distinct.append(products(f, s, max_level=max_level, levels=self.levels, weights=self.wts[-1]))
        self.n_seeds_of = np.array([len(p.ps) for p in self.distinct], dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.n_seeds_of[self.which])])
        self.cube = np.stack(self.imgs)[self.which]
        self.weights = np.stack(self.wts)[self.which]
        self.seeds = np.concatenate([self.distinct[k].ps for k in self.which], axis=0)

    def planes(self, what):
        """(n, h, w) u32: what(products) of every slice."""
        return np.stack([what(p) for p in self.distinct])[self.which]

    def records(self, what):
        """The slices' per-colour records (S_k + 1 each) one after the other, as the batch calls lay them out."""
        per = [what(p) for p in self.distinct]
        return np.concatenate([per[k] for k in self.which], axis=0)

    def lists(self, merging):
        """(counts (n * levels), records (total, 2) colour / area, uncoloured (n * levels)): bin k * levels + l holds slice k's
        lakes at level l, colours ascending."""
        levels = self.max_level + 1
        cnt, rec, unc = [], [], []
        for p in self.distinct:
            lk = p.lakes if merging else p.seg_lakes
            cnt.append(np.array([len(c) for c, _, _ in lk], dtype=np.int64))
            unc.append(np.array([u for _, _, u in lk], dtype=np.int64))
            rec.append(np.concatenate([np.stack([c, a], axis=1).astype(np.int64).reshape(-1, 2) for c, a, _ in lk], axis=0))
        counts = np.stack(cnt)[self.which].reshape(self.n * levels)
        uncol = np.stack(unc)[self.which].reshape(self.n * levels)
        return counts, np.concatenate([rec[k] for k in self.which], axis=0), uncol
