"""Seed lists that are dense, adjacent or clustered, and images whose maxima are: the inputs of tests/test_gpu_seed_regimes.py.

Nearly every other GPU test seeds its transform with the local maxima of a noise field (never adjacent: no mask nibble with two
neighbouring bits) or with a random list of one seed per ten pixels at the most.  The seed kernels work in units that only dense
lists fill: the nibble (four pixels of a row: the resolve's seed colours), the 32-pixel mask word, the 256-pixel paint segment,
the paint chunk of 4096 and the table chunk of 8192 pixels, the 1024-entry stage of the minima compaction.  Pure numpy, seeded;
tests/test_seed_cases_cpu.py proves on the oracle and on numpy that the cases reach what `facts` claims.

A segmenting case is (name, image, seeds, facts): seeds an (n, 2) int64 array of (row, col), facts a dict
  family  "S1" .. "S7" (see segment_cases)
  strict  the list is strictly increasing in row-major order
  form    "tables" (strict, W % 4 == 0: the seed side tables) or "painted" (everything else: the painted label plane)
A minima case is (name, image, facts): facts holds `family` ("M1" .. "M5"), `want` (the strict interior maxima by construction,
row-major, where the construction gives them: else None) and, for a view into a larger buffer, `offset` and `row_stride`.
"""
import numpy as np

import cases

NIBBLE = 4
WORD = 32              # pixels per mask word
PAINT_SEG = 256        # pixels per step of a painting wave
PAINT_CHUNK = 4096     # pixels per painting wave
TAB_CHUNK = 8192       # pixels per wave of the seed tables
MINIMA_STEP = 64       # 32-pixel groups per step of the compaction's wave: 1024 list entries at the most

SHAPES = {"A": (72, 136),      # W % 4 == 0, W % 32 != 0
          "B": (64, 160),      # W % 32 == 0, stackable (H * W % 128 == 0)
          "C": (67, 131),      # odd: always the painted form and the scalar resolve branch
          "D": (130, 260),     # several tiles each way, five table chunks
          "E": (3, 2736),      # thin planes that still span two table chunks
          "F": (2740, 3),
          "G": (64, 260)}      # one of the small planes the seam-repair tests force that flow on


# ---- images -----------------------------------------------------------------------------------------------------------------------

def image(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return cases.field(h, w, seed)
    if kind == "plateau":      # four values: long ties, arrival rings in every direction
        return (rng.integers(0, 4, (h, w)) * 60).astype(np.uint8)
    if kind == "walls":        # NEVER_FILL walls with gaps, ALWAYS_FILL floors
        img = rng.integers(0, 254, (h, w), dtype=np.uint8)
        img[rng.random((h, w)) < 0.15] = 255
        img[rng.random((h, w)) < 0.15] = 0
        img[:, w // 3] = 255
        img[h // 2, :] = 255
        img[h // 2, w // 2] = 0
        return img
    raise ValueError(kind)


KINDS = ("noise", "plateau", "walls")


# ---- seed lists -------------------------------------------------------------------------------------------------------------------

def from_pixels(px, w):
    px = np.asarray(px, dtype=np.int64)
    return np.stack([px // w, px % w], axis=1)


def pixels_of(seeds, w):
    s = np.asarray(seeds, dtype=np.int64).reshape(-1, 2)
    return s[:, 0] * w + s[:, 1]


def is_strict(seeds, w):
    p = pixels_of(seeds, w)
    return bool((p[1:] > p[:-1]).all())


def shuffled(seeds, seed):
    s = np.asarray(seeds, dtype=np.int64).reshape(-1, 2)
    return np.ascontiguousarray(s[np.random.default_rng(seed).permutation(len(s))])


def then_reversed(seeds):
    """The list followed by a reversed copy of itself: every pixel twice, the later entry wins (lib.rs:1672-1677)."""
    s = np.asarray(seeds, dtype=np.int64).reshape(-1, 2)
    return np.ascontiguousarray(np.concatenate([s, s[::-1]]))


def bernoulli(h, w, density, seed):
    return from_pixels(np.flatnonzero(np.random.default_rng(seed).random(h * w) < density), w)


def _case(out, name, key, kind, seeds, family):
    h, w = SHAPES[key]
    seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.int64).reshape(-1, 2))
    strict = is_strict(seeds, w)
    facts = {"family": family, "strict": strict, "form": "tables" if strict and w % 4 == 0 and len(seeds) else "painted", "shape": key}
    out.append((f"{family}/{key}/{name}/{kind}", image(kind, h, w, 1000 + len(out)), seeds, facts))


_SEGMENT = None


def segment_cases():
    """Every S case.  The image kind rotates through noise, plateau and walls."""
    global _SEGMENT
    if _SEGMENT is not None:
        return _SEGMENT
    out = []

    def kind():
        return KINDS[len(out) % 3]

    # S1 every pixel, row-major
    for key in "ABCDEF":
        h, w = SHAPES[key]
        _case(out, "all", key, kind(), from_pixels(np.arange(h * w), w), "S1")
    # S2 Bernoulli 1/2 and 7/8, sorted
    for key in "ABCDEF":
        h, w = SHAPES[key]
        _case(out, "half", key, kind(), bernoulli(h, w, 0.5, 11 + h), "S2")
    for key in "ACDG":
        h, w = SHAPES[key]
        _case(out, "seven_eighths", key, kind(), bernoulli(h, w, 0.875, 13 + h), "S2")
    _case(out, "half", "G", kind(), bernoulli(64, 260, 0.5, 11 + 64), "S2")
    # S3 solid blocks
    for key in "ABCG":
        h, w = SHAPES[key]
        px = np.arange(h * w)
        r, c = px // w, px % w
        _case(out, "rows", key, kind(), from_pixels(px[np.isin(r, (0, 1, h // 2, h // 2 + 1, h - 1))], w), "S3")
        _case(out, "columns", key, kind(), from_pixels(px[np.isin(c, (0, 1, w - 1))], w), "S3")
    h, w = SHAPES["D"]
    px = np.arange(h * w)
    in_chunk1 = (px >= TAB_CHUNK) & (px < 2 * TAB_CHUNK)
    _case(out, "chunk1", "D", kind(), from_pixels(px[in_chunk1], w), "S3")                  # chunks 0 and 2 stay empty
    _case(out, "all_but_chunk1", "D", kind(), from_pixels(px[~in_chunk1], w), "S3")
    # S4 runs that straddle a table chunk and sit on the boundaries of the 64-ary search
    for key, lengths in (("D", (64, 65, 256, 257, 4096, 4097)), ("A", (64, 65, 256, 257))):
        h, w = SHAPES[key]
        for n in lengths:
            _case(out, f"run{n}", key, kind(), from_pixels(np.arange(TAB_CHUNK - 31, TAB_CHUNK - 31 + n), w), "S4")
    # S5 the ends of the plane
    for key in "CDEF":
        h, w = SHAPES[key]
        assert (h * w) % WORD
        _case(out, "last_word", key, kind(), from_pixels(np.arange(h * w - (h * w) % WORD, h * w), w), "S5")
    for key in "AC":
        h, w = SHAPES[key]
        _case(out, "pixel0", key, kind(), from_pixels([0], w), "S5")
        _case(out, "last_pixel", key, kind(), from_pixels([h * w - 1], w), "S5")
    # S6 S1, S2 and S3 shuffled, and sorted followed by their reverse (n > H * W for S1)
    for key in "AC":
        h, w = SHAPES[key]
        px = np.arange(h * w)
        lists = (("all", from_pixels(px, w)), ("half", bernoulli(h, w, 0.5, 11 + h)),
                 ("rows", from_pixels(px[np.isin(px // w, (0, 1, h // 2, h // 2 + 1, h - 1))], w)))
        for tag, s in lists:
            _case(out, f"{tag}_shuffled", key, kind(), shuffled(s, 17 + len(out)), "S6")
            _case(out, f"{tag}_then_reversed", key, kind(), then_reversed(s), "S6")
    # S7 sorted with one repeated entry in the middle: not strict, the tables must refuse it
    for key in "ACD":
        h, w = SHAPES[key]
        s = bernoulli(h, w, 0.5, 19 + h)
        mid = len(s) // 2
        _case(out, "one_repeat", key, kind(), np.concatenate([s[:mid + 1], s[mid:]]), "S7")
    _SEGMENT = out
    return out


def by_family(*families, shape=None):
    return [c for c in segment_cases() if c[3]["family"] in families and (shape is None or c[3]["shape"] in shape)]


def case_named(prefix):
    got = [c for c in segment_cases() if c[0].startswith(prefix)]
    assert len(got) == 1, (prefix, [c[0] for c in got])
    return got[0]


# ---- what a list reaches (numpy; the CPU test asserts these) ------------------------------------------------------------------------

def seed_mask(seeds, shape):
    """One bool per pixel, row-major."""
    m = np.zeros(shape[0] * shape[1], dtype=bool)
    m[pixels_of(seeds, shape[1])] = True
    return m


def nibbles_by_position(seeds, shape):
    """counts[pos, pattern]: how often nibble `pattern` (bit k: pixel 4 j + k of the row is a seed) occurs at nibble position
    `pos` (0 .. 7) of a mask word, for W % 4 == 0."""
    h, w = shape
    assert w % NIBBLE == 0
    m = seed_mask(seeds, shape).reshape(-1, NIBBLE)
    pat = (m * (1 << np.arange(NIBBLE))).sum(axis=1)
    pos = np.arange(len(pat)) % (WORD // NIBBLE)
    counts = np.zeros((WORD // NIBBLE, 16), dtype=np.int64)
    np.add.at(counts, (pos, pat), 1)
    return counts


def per_unit(seeds, shape, unit):
    """Seeds in every aligned run of `unit` pixels (the last one may be short)."""
    m = seed_mask(seeds, shape)
    pad = (-len(m)) % unit
    return np.concatenate([m, np.zeros(pad, dtype=bool)]).reshape(-1, unit).sum(axis=1)


def painted(seeds, shape):
    """The seed plane by the rule itself: colour i + 1 at seed i, later entries overwrite (lib.rs:1670-1677)."""
    out = np.zeros(shape[0] * shape[1], dtype=np.uint64)
    out[pixels_of(seeds, shape[1])] = np.arange(1, len(seeds) + 1, dtype=np.uint64)      # (numpy assigns in order: the last one stays)
    return out.reshape(shape)


# ---- images whose maxima are the case -----------------------------------------------------------------------------------------------

PEAK_FLOOR = ((1, 0), (255, 254), (200, 10))       # 254 and 255: bytes no generated field holds

MINIMA_SHAPES = ((9, 2080), (9, 2084), (40, 2049),      # a full 64-lane step: aligned W % 32, aligned W % 4, unaligned
                 (66, 130), (33, 1056), (3, 1024), (3, 1028), (5, 4), (5, 8), (3, 3))


def strict_maxima(img):
    """Strict 8-neighbour maxima of the interior, row-major, by eight shifted comparisons (lib.rs:1178-1197 restated)."""
    a = np.asarray(img).astype(np.int64)
    h, w = a.shape
    if h < 3 or w < 3:
        return np.zeros((0, 2), dtype=np.int64)
    c = a[1:-1, 1:-1]
    ok = np.ones(c.shape, dtype=bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                ok &= c > a[dy:dy + h - 2, dx:dx + w - 2]
    r, x = np.nonzero(ok)
    return np.stack([r + 1, x + 1], axis=1).astype(np.int64)


def _lattice(h, w, first):
    """Interior lattice points (first, first + 2, ...) in both directions, row-major."""
    rr, cc = np.arange(first, h - 1, 2), np.arange(first, w - 1, 2)
    if len(rr) == 0 or len(cc) == 0:
        return np.zeros((0, 2), dtype=np.int64)
    g = np.stack(np.meshgrid(rr, cc, indexing="ij"), axis=-1).reshape(-1, 2)
    return g.astype(np.int64)


def _put(img, pts, v):
    if len(pts):
        img[pts[:, 0], pts[:, 1]] = v


def m1(h, w, peak, floor):
    img = np.full((h, w), floor, dtype=np.uint8)
    pts = _lattice(h, w, 1)
    _put(img, pts, peak)
    return img, pts


def m2(h, w, peak, floor):
    img = np.full((h, w), floor, dtype=np.uint8)
    pts = _lattice(h, w, 2)
    _put(img, pts, peak)
    return img, pts


def m3(h, w, peak, floor):
    """M1 with every third peak lowered to a value its right neighbour shares, and every fifth (of the others) to one its
    lower-right neighbour shares: neither is strict any more.  The shared value is half way up (the peak's own where the
    peak stands one above the floor: then the raised neighbour also ties with the next peak, and `want` is None)."""
    img, pts = m1(h, w, peak, floor)
    tie = floor + (peak - floor + 1) // 2
    k = np.arange(len(pts))
    third, fifth = k % 3 == 2, (k % 5 == 4) & (k % 3 != 2)
    for sel, dy in ((third, 0), (fifth, 1)):
        p = pts[sel]
        _put(img, p, tie)
        _put(img, p + np.array([dy, 1]), tie)
    return img, (pts[~(third | fifth)] if tie < peak else None)


def m4(h, w, peak, floor):
    """Peaks on the border rows and columns (never reported) and on row 1, row H - 2, column 1 and column W - 2 (reported), and M1's
    lattice further in.  A peak is placed only where no 8-neighbour holds one already, so every interior one placed is strict."""
    img = np.full((h, w), floor, dtype=np.uint8)
    cand = []
    for r in (0, h - 1):
        cand += [(r, c) for c in range(3, w, 4)]
    for c in (0, w - 1):
        cand += [(r, c) for r in range(3, h, 4)]
    for r in (1, h - 2):
        cand += [(r, c) for c in range(1, w - 1, 4)]
    for c in (1, w - 2):
        cand += [(r, c) for r in range(1, h - 1, 4)]
    cand += [(r, c) for r in range(3, h - 3, 2) for c in range(3, w - 3, 2)]
    placed = np.zeros((h + 2, w + 2), dtype=bool)
    for r, c in cand:
        if 0 <= r < h and 0 <= c < w and not placed[r:r + 3, c:c + 3].any():
            placed[r + 1, c + 1] = True
    inner = placed[1:-1, 1:-1]
    img[inner] = peak
    interior = inner.copy()
    interior[0, :] = interior[-1, :] = False
    interior[:, 0] = interior[:, -1] = False
    r, c = np.nonzero(interior)
    facts_border = int(inner.sum() - interior.sum())
    return img, np.stack([r, c], axis=1).astype(np.int64), facts_border


def m5(h, w, peak, floor):
    """Staggered: odd columns on rows = 1 mod 4, even columns on rows = 3 mod 4."""
    img = np.full((h, w), floor, dtype=np.uint8)
    pts = [(r, c) for r in range(1, h - 1) if r % 4 in (1, 3) for c in range(1 if r % 4 == 1 else 2, w - 1, 2)]
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
    _put(img, pts, peak)
    return img, pts


_MINIMA = None


def minima_cases():
    global _MINIMA
    if _MINIMA is not None:
        return _MINIMA
    out = []
    for (h, w) in MINIMA_SHAPES:
        for family, make in (("M1", m1), ("M2", m2), ("M3", m3), ("M4", m4), ("M5", m5)):
            # all three (peak, floor) pairs on the smallest full-step shape and the small ones; one pair, rotating, elsewhere
            pairs = PEAK_FLOOR if (h, w) in ((9, 2080), (66, 130), (5, 8)) else (PEAK_FLOOR[(h + w + len(out)) % 3],)
            for peak, floor in pairs:
                res = make(h, w, peak, floor)
                facts = {"family": family, "want": res[1], "peak": peak, "floor": floor}
                if family == "M4":
                    facts["border_peaks"] = res[2]
                out.append((f"{family}/{h}x{w}/{peak}over{floor}", res[0], facts))
    # one view into a larger buffer: a 1-byte offset and a row stride that is not W
    img, pts = m1(9, 2080, 255, 254)
    out.append(("M1/9x2080/255over254/offset1", img, {"family": "M1", "want": pts, "peak": 255, "floor": 254, "offset": 1, "row_stride": 2080 + 7}))
    _MINIMA = out
    return out


def minima_named(prefix):
    got = [c for c in minima_cases() if c[0].startswith(prefix)]
    assert got, prefix
    return got[0]
