"""Inputs that put the merging transform's per-level products under load, in plain numpy (seeded, no GPU), and what the CPU
oracle says about each: tests/test_merging_cases_cpu.py proves from the oracle's records that the inputs reach the regimes,
tests/test_gpu_merging_products_random.py compares the engine's history planes, lake lists, merge tree and lake catalogue with
them bit for bit.

Field kinds, as tests/test_gpu_random_cases.py draws them: `few` (integers(0, 6) * k: big plateaus, mass merges at six levels),
`walls` (choice([0, 255, a, b]): NEVER_FILL walls, ALWAYS_FILL floors, seeds on both), `ramp` (+ noise), `constant`, `noise` (the
control).  Seed-list forms: `sorted` (strictly increasing, row-major), `shuffled` (the same list permuted: the painted plane),
`repeats` (every n-th entry again at the end: the earlier colour of each pair does not exist), `borders` (corners, border pixels,
vertically and horizontally adjacent seeds).  Constructed fields: the staircase, the seeded plateaus, the two seas."""
import os
import zlib
from dataclasses import dataclass
from typing import Optional

import numpy as np

import lake_stats_ref as ls
import merge_tree_ref as mt
import oracle_lib as ol

KINDS = ("few", "walls", "ramp", "constant", "noise")
FORMS = ("sorted", "shuffled", "repeats", "borders")


def seed_offset():
    """WS_TEST_SEED_OFFSET: ad-hoc wider sweeps, as tests/test_gpu_random_cases.py."""
    return int(os.environ.get("WS_TEST_SEED_OFFSET", "0"))


class Case:
    """One call: image, seed list, options, and the level list its history is asked for."""

    def __init__(self, name, img, seeds, kind, form, max_level=254, edge=False, seed_shift=False, levels=None):
        self.name = name
        self.img = np.ascontiguousarray(img, dtype=np.uint8)
        self.seeds = np.asarray(seeds, dtype=np.int64).reshape(-1, 2)
        self.kind, self.form = kind, form
        self.max_level, self.edge, self.seed_shift = int(max_level), bool(edge), bool(seed_shift and edge)
        self.levels = list(range(self.max_level + 1)) if levels is None else [int(l) for l in levels]

    @property
    def plane_shape(self):
        e = 2 if self.edge else 0
        return self.img.shape[0] + e, self.img.shape[1] + e

    def __repr__(self):
        h, w = self.img.shape
        return (f"{self.name}[{h}x{w} {self.kind}/{self.form} seeds={len(self.seeds)} max={self.max_level} edge={int(self.edge)}"
                f" shift={int(self.seed_shift)}]")


def make_field(kind, h, w, rng, k=40):
    if kind == "few":
        return (rng.integers(0, 6, (h, w), dtype=np.uint8) * k).astype(np.uint8)
    if kind == "walls":
        a, b = (17, 200) if k >= 40 else (1, k)
        return rng.choice(np.array([0, 255, a, b], dtype=np.uint8), (h, w), p=[0.3, 0.2, 0.3, 0.2])
    if kind == "ramp":
        return ((np.add.outer(np.arange(h), np.arange(w)) * 3 + rng.integers(0, 9, (h, w))) % 254).astype(np.uint8)
    if kind == "constant":
        return np.full((h, w), k, dtype=np.uint8)
    assert kind == "noise", kind
    return rng.integers(0, 254, (h, w), dtype=np.uint8)


def make_seeds(form, h, w, n, rng, every=7):
    """(n', 2) int64 (row, col) pairs of the form asked for, from n distinct pixels drawn at random."""
    n = max(1, min(n, h * w))
    flat = np.sort(rng.choice(h * w, size=n, replace=False))
    if form == "borders":
        near = flat[:: 5]
        right = near[(near % w) < w - 1] + 1                      # horizontally adjacent pairs
        below = near[1:: 2][(near[1:: 2] // w) < h - 1] + w       # vertically adjacent pairs
        corners = np.array([0, w - 1, (h - 1) * w, h * w - 1])
        rows, cols = rng.integers(0, h, 12), rng.integers(0, w, 12)
        border = np.concatenate([cols, (h - 1) * w + cols, rows * w, rows * w + w - 1])
        flat = np.unique(np.concatenate([flat, right, below, corners, border]))
    seeds = np.stack([flat // w, flat % w], axis=1).astype(np.int64)
    if form == "shuffled":
        seeds = seeds[rng.permutation(len(seeds))]
    elif form == "repeats":
        seeds = np.concatenate([seeds, seeds[:: every]])
    return seeds


def level_list(max_level, rng):
    """An unsorted level list with repeats that holds 0 and max_level."""
    lv = [int(x) for x in rng.integers(0, max_level + 1, 5)] + [0, max_level]
    lv.append(lv[int(rng.integers(0, len(lv)))])
    while True:
        out = [lv[i] for i in rng.permutation(len(lv))]
        if out != sorted(out):
            return out


# kind, k, form, rows, columns (a multiple of 4, or odd), pixels per seed, max_level, edge, seed_shift
_SWEEP = [
    ("few", 3, "repeats", (300, 331), (700, 801, 4), 52, 254, False, False),
    ("few", 3, "sorted", (190, 211), (500, 541, 4), 35, 17, True, True),
    ("walls", 40, "shuffled", (250, 300), (600, 700, 4), 60, 254, False, False),
    ("ramp", 0, "borders", (257, 300), (161, 260, 1), 45, 254, True, True),
    ("constant", 0, "repeats", (120, 140), (500, 560, 4), 30, 100, False, False),      # every pixel floods at level 0
    ("noise", 0, "sorted", (130, 170), (240, 300, 4), 12, 254, False, False),          # the control
    ("few", 1, "borders", (3, 9), (700, 801, 4), 6, 17, True, False),                  # a strip: one row of tiles
    ("walls", 1, "sorted", (300, 331), (501, 640, 1), 25, 1, False, False),            # two levels
    ("few", 40, "shuffled", (200, 260), (400, 520, 4), 70, 254, True, False),
    ("few", 20, "repeats", (257, 330), (513, 700, 4), 40, 100, False, False),
    ("constant", 3, "borders", (64, 130), (257, 400, 4), 20, 17, True, True),
    ("few", 2, "sorted", (129, 200), (385, 600, 1), 30, 17, False, False),             # rows and columns odd: an odd pixel count
]


def sweep_cases():
    """The sweep of single fields: shapes of up to 5 x 4 relaxation tiles of 256 x 64 with ragged last tiles, every fourth
    width no multiple of 4, every option drawn.  The regimes are planned per slot (this table); contents, shapes within the
    slot's range, seed positions and level lists come from the generator."""
    rng = np.random.default_rng(31337 + seed_offset())
    out = []
    for i, (kind, k, form, rows, (lo, hi, mult), per, max_level, edge, shift) in enumerate(_SWEEP):
        h = int(rng.integers(*rows))
        w = int(rng.integers(lo, hi))
        w = w // 4 * 4 if mult == 4 else w | 1
        if mult == 1 and i == len(_SWEEP) - 1:
            h |= 1
        img = make_field(kind, h, w, rng, k)
        seeds = make_seeds(form, h, w, h * w // per, rng)
        out.append(Case(f"sweep{i}", img, seeds, kind, form, max_level, edge, shift, level_list(max_level, rng)))
    return out


def staircase():
    """257 x 260, a wall ring, interior row r at min(h - 2 - r, 254), one seed per interior row at a varying column: every
    level floods one more row above the lake, which there touches the seed pixel of the row above that and takes its smaller
    colour as canonical id -- colour c dies at level 255 - c into c - 1, a parent chain 254 deep."""
    h, w = 257, 260
    img = np.full((h, w), 255, dtype=np.uint8)
    rows = np.arange(1, h - 1)
    img[1:-1, 1:-1] = np.minimum(h - 2 - rows, 254)[:, None]
    seeds = np.stack([rows, 1 + (rows * 37) % (w - 2)], axis=1)
    return Case("staircase", img, seeds, "staircase", "sorted")


def seeded_plateau(w):
    """A floor of 130 rows at value 0 with a seed on every third pixel: with w % 3 == 0 the seeds stack in columns.  Its history
    is asked for at all 18 levels."""
    h = 130
    flat = np.arange(0, h * w, 3)
    return Case(f"plateau_w{w}", np.zeros((h, w), dtype=np.uint8), np.stack([flat // w, flat % w], axis=1), "plateau", "sorted",
                max_level=17)


TWO_SEAS_V = 40


def two_seas(max_level):
    """Two seas, 298 x 320 and 298 x 321 pixels (four values below v, 0/13/26/39, some 150 seeds each), inside walls and joined
    by ONE pixel of value v.  Its history is asked for at every level up to max_level: the mass merges at 13 and 26, the join
    at v, and the planes that must not change in between."""
    v = TWO_SEAS_V
    h, w = 300, 644
    rng = np.random.default_rng(5)
    img = np.full((h, w), 255, dtype=np.uint8)
    img[1:-1, 1:321] = rng.integers(0, 4, (h - 2, 320), dtype=np.uint8) * (v // 4 + 3)
    img[1:-1, 322:643] = rng.integers(0, 4, (h - 2, 321), dtype=np.uint8) * (v // 4 + 3)
    img[77, 321] = v
    flat = np.sort(rng.choice(h * w, size=400, replace=False))
    seeds = np.stack([flat // w, flat % w], axis=1)
    seeds = seeds[img[seeds[:, 0], seeds[:, 1]] != 255]
    return Case(f"two_seas_max{max_level}", img, seeds, "two_seas", "sorted", max_level=max_level)


def constructed_cases():
    v = TWO_SEAS_V
    return [staircase(), seeded_plateau(516), seeded_plateau(517), two_seas(v - 1), two_seas(v), two_seas(254)]


# slices, rows, columns of the padded plane (it stacks if w' % 4 == 0 and h' * w' % 128 == 0), edge, max_level, which slice
# is shuffled (the whole call then takes the loop), pixel limit in planes (0: none)
_CUBES = [
    (6, 128, 96, False, 254, None, 0),
    (5, 264, 128, True, 17, None, 2),          # groups of 2 + 2 + 1; slices of more than one tile
    (4, 130, 98, False, 100, None, 0),         # no stack: w' % 4 != 0
    (5, 96, 132, True, 254, 2, 0),             # a shuffled list
    (3, 40, 96, False, 1, None, 0),            # 3840 pixels: the runs of the own-count pass straddle slices
    (6, 65, 131, False, 17, None, 3),          # no stack, odd pixel count
    (4, 64, 260, False, 254, 1, 3),            # shuffled list and groups
    (5, 200, 64, True, 100, None, 0),
]


def cube_cases():
    """Stacks of 3 to 6 slices of mixed kinds, one seedless slice each: [(slices: list of Case, pixel limit)]."""
    rng = np.random.default_rng(4711 + seed_offset())
    out = []
    for i, (s, ph, pw, edge, max_level, shuffled, limit) in enumerate(_CUBES):
        h, w = (ph - 2, pw - 2) if edge else (ph, pw)
        seedless = int(rng.choice([k for k in range(s) if k != shuffled]))
        levels = level_list(max_level, rng)
        slices = []
        for k in range(s):
            kind = KINDS[int(rng.integers(0, len(KINDS)))]
            kk = {"few": 3 if max_level >= 17 else 1, "walls": 40 if max_level > 200 else 1, "constant": int(rng.integers(0, 2))}.get(kind, 0)
            form = "shuffled" if k == shuffled else ("sorted", "repeats", "borders")[int(rng.integers(0, 3))]
            seeds = make_seeds(form, h, w, h * w // int(rng.integers(8, 40)), rng)
            if k == seedless:
                seeds, form = seeds[:0], "none"
            slices.append(Case(f"cube{i}.{k}", make_field(kind, h, w, rng, kk), seeds, kind, form, max_level, edge, False, levels))
        out.append((slices, limit * ph * pw))
    return out


def weight_planes(shape, seed):
    """The three weight choices of tests/test_gpu_lake_stats.py (_weight_planes): none (the image: on a six-level field almost every
    peak is a tie), a u8 plane, and a u16 plane that holds 0 and 65535 several times each."""
    rng = np.random.default_rng(1000 + seed)
    u8 = rng.integers(0, 256, shape, dtype=np.uint8)
    u16 = rng.integers(0, 65536, shape, dtype=np.uint16)
    flat = u16.reshape(-1)
    where = rng.permutation(flat.size)
    flat[where[:max(flat.size // 50, 2)]] = 65535
    flat[where[-max(flat.size // 50, 2):]] = 0
    return [("image", None), ("u8", u8), ("u16", u16)]


@dataclass
class Expected:
    """What the oracle says about one case, kept small.  S: the number of seeds; every per-colour array has S + 1 entries,
    entry 0 for the uncoloured pixels."""
    ps: np.ndarray                      # (S, 2) the seeds in coordinates of the padded plane
    parent: np.ndarray                  # u32: the colour this one died into, 0 while alive
    death: np.ndarray                   # u32: the level it died at, merge_tree_ref.ALIVE while alive
    area: np.ndarray                    # u32: pixels at death, or at max_level; [0]: uncoloured at max_level
    leaves: np.ndarray                  # u32: existing seeds it holds then; 0 for a colour that never was
    vals: np.ndarray                    # (levels, S + 1) int64: P_L at each colour's seed pixel
    ex: np.ndarray                      # bool: the colour exists (its seed pixel was not painted over by a duplicate)
    tree: np.ndarray                    # (S + 1, 4) parent, death, area, leaves as the engine's records
    lakes: list                         # per level 0..max_level: (colours ascending, their areas, uncoloured pixels)
    planes: dict                        # level -> canonical merging plane, for the levels of case.levels
    labels: np.ndarray                  # u32 plane: ol.segment_arrival, what merge_tree's want_labels gives
    weights: Optional[list] = None      # [(name, plane or None)]: weight_planes(), where the catalogue was asked for
    stats: Optional[dict] = None        # name -> lake_stats_ref records under that weight plane
    seg_planes: Optional[dict] = None   # level -> segmenting plane (ol.segment's hook), where asked for


_CACHE = {}


def _key(case):
    """Name, seed offset and a checksum of the inputs: two cases that share a name by mistake never share an entry."""
    return case.name, seed_offset(), case.max_level, case.edge, case.seed_shift, zlib.crc32(case.seeds.tobytes(), zlib.crc32(case.img.tobytes()))


def _plane(p, n_seeds):
    """A plane of colours 0..n_seeds in the narrowest unsigned type that holds them: a constructed case keeps every level."""
    assert p.min() >= 0 and p.max() <= n_seeds
    return p.astype(np.uint16 if n_seeds < 1 << 16 else np.uint32)


def expected(case, want_stats=True, want_segmenting=True):
    """Everything from ONE run of the merging oracle (and one of the segmenting oracle for its history planes), computed once
    per process and case and never changed afterwards; a later call that wants more than the entry holds computes it anew."""
    key = _key(case)
    hit = _CACHE.get(key)
    if hit is not None and (hit.stats is not None or not want_stats) and (hit.seg_planes is not None or not want_segmenting):
        return hit
    planes, ps = mt.oracle_planes(case.img, case.seeds, case.max_level, case.edge, case.seed_shift)
    parent, death, area, leaves, vals, ex = mt.tree_from_planes(planes, ps)
    lakes = []
    for P in planes:
        hist = ol.find_lake_sizes(P)
        cols = np.flatnonzero(hist[1:]) + 1
        lakes.append((cols, hist[cols], int(hist[0])))
    want = set(case.levels)
    e = Expected(ps=ps, parent=parent, death=death, area=area, leaves=leaves, vals=vals, ex=ex,
                 tree=np.stack([parent, death, area, leaves], axis=1), lakes=lakes,
                 planes={L: _plane(planes[L], len(ps)) for L in want},
                 labels=ol.segment_arrival(case.img, ps, max_level=case.max_level, edge=case.edge).astype(np.uint32))
    if want_stats:
        e.weights = weight_planes(case.img.shape, len(case.seeds))
        e.stats = {name: ls.stats_from_planes(planes, ps, ls.plane_weights(case.img, wt, case.edge), death, ex) for name, wt in e.weights}
    del planes
    if want_segmenting:
        keep = {}
        ol.segment(case.img, ps, max_level=case.max_level, edge=case.edge,
                   hook=lambda l, m, i, c: keep.__setitem__(int(l), _plane(c, len(ps))) if int(l) in want else None)
        e.seg_planes = keep
    _CACHE[key] = e
    return e


def describe(case, e):
    """The regime a case reaches, from the oracle's records: the row of the table in the pull request."""
    dead = e.death != mt.ALIVE
    per_level = np.bincount(e.death[dead].astype(np.int64), minlength=256)
    depth = np.zeros(e.parent.size, dtype=np.int64)
    for c in np.flatnonzero(dead):          # parent < c: a parent's depth is final before its children's
        depth[c] = depth[e.parent[c]] + 1
    alive = ~dead & e.ex
    v = ls.plane_weights(case.img, None, case.edge)      # the image over the padded plane
    on_wall = alive[1:] & (v[e.ps[:, 0], e.ps[:, 1]] == 255) & (e.area[1:] == 1)
    return {"name": case.name, "shape": case.img.shape, "kind": case.kind, "form": case.form, "max_level": case.max_level,
            "edge": case.edge, "seed_shift": case.seed_shift, "seeds": len(e.ps), "nonexistent": int((~e.ex[1:]).sum()),
            "most_deaths": int(per_level.max()), "busiest_level": int(per_level.argmax()), "deaths_at_0": int(per_level[0]),
            "largest_lake": int(e.area[1:].max()) if len(e.ps) else 0, "depth": int(depth.max()),
            "survivors": int(alive.sum()), "survivors_on_255_area_1": int(np.sum(on_wall))}
