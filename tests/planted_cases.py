"""Planted stamp planes: start states of the relaxation that no flood from seeds produces, and their exact fixpoint.

ws_block_relax (and ws_block_begin + ws_block_relax_halo, from the halo rows) take the caller's key plane as the start state
and relax it to the fixpoint of  t <- min(t, max(b, 1 + min4)).  From ANY start plane T0 that fixpoint is unique (border
pixels and pixels above the maximum level are pinned; induction over the pixels in order of their final value), so a heap
Dijkstra over (level, ring) pairs gives it exactly -- with no 24-bit ring field, which is how small planes reach what a flood
from seeds needs a corridor of 16.7 M pixels for: rings at the top of the field, the carry guard, and the scans' arithmetic
on large numbers.  Inputs of tests/test_gpu_planted_stamps.py; tests/test_planted_cases_cpu.py proves on the CPU that every
family reaches what it claims.

A case is (img, t0, max_level): img uint8, t0 uint32.  A planted stamp is 0 (a seed), KEY_INF (never coloured) or
(level << 24) | ring with 1 <= ring <= LAST_RING: never a finite stamp with ring 0 and never ring 2^24 - 1 -- the kernels'
write-back test reads whole patches, planted pixels included, and those two are what it refuses.

THE CONTRACT (include/ws_hip.h, WS_ERR_RING_OVERFLOW): a flood may reach ring LAST_RING = 2^24 - 2 inside one level; one
that reaches 2^24 - 1 is refused.  (Refusing only the carry itself, ring 2^24, left a hole at level 254: 0xFEFFFFFF + 1 is
KEY_INF, "never coloured", and nothing was reported.)

Families (every generator is deterministic):
  rows        walls with one-pixel corridors on every second row, each fed from a planted stamp on its border pixel in
              column 0 or, alternately, column W - 1, each with one blocker: a pixel of a higher level (9, 200, 254: the flood
              goes on at that level -- the clamp by b), a wall (the far side stays KEY_INF), or a wall with a second planted
              stamp at the other end (two fronts, one from each side of the blocker).  Blocker columns cover, per direction,
              every residue x mod 256 of LANE_RESIDUES: the DPP row ends, the row_bcast / readlane hand-overs at lanes
              16 / 32 / 48 and the half-row boundary of the 128-wide tiles.  776 x 131 (W % 4 == 0, last tile column partial)
              and 774 x 131 (the scalar write-back of the general form).
  columns     the transpose: corridors on every second column, fed from row 0 or row H - 1, blocker rows covering every
              residue y mod 64 per direction -- all patch rows of all bands of the 32- and 64-row tiles.  260 x 200.  Only the
              first and the last row hold planted stamps, so the same plane is what ws_block_relax_halo starts from.
  high rings  rows and columns with every source's ring raised until the last pixel its flood reaches holds exactly LAST_RING,
              at levels 7 and 254, and at level 253 with max_level 253 (the other patch_bases path).  Corridors are single
              paths from KEY_INF: no transient stamp exceeds the fixpoint's, so the kernels must not report a carry.
  twins       a high-ring plane with ONE source one ring higher: exactly one pixel needs ring 2^24 - 1.
  random      33 .. 70 rows, 250 .. 530 columns, both W % 4 classes; bytes from {3, 7, 7, 7, 9, 200, 254, 255}; 15 % of ALL
              pixels hold a planted stamp of a random level, 2 % hold 0; max_level 254 or 100.  Rings come from
              {1, 2, 100, R}, R = min(0xFFF000, 2^24 - 2 - H * W): ring + pixel count stays below 2^24 - 1, so no transient can
              reach the refused ring (a stamp is its source's ring plus the length of a SIMPLE path: stamps only fall, so a
              chain of assignments never revisits a pixel).  0xFFF000 itself satisfies that for no shape of the family (the
              smallest plane has 8250 pixels, 0xFFF000 leaves room for 4094), hence the cap.
"""
import functools
import heapq

import numpy as np

KEY_INF = 0xFF000000
RING_MASK = 0x00FFFFFF
LAST_RING = 0xFFFFFE          # the last ring a flood may reach inside one level (see THE CONTRACT above)

LANE_RESIDUES = tuple(4 * lane + c for lane in (0, 15, 16, 31, 32, 47, 48, 63) for c in range(4))      # x mod 256
BAND_RESIDUES = tuple(range(64))                                                                        # y mod 64
BLOCKER_LEVELS = (9, 200, 254)
KIND_LEVEL, KIND_WALL, KIND_WALL_TWO_FRONTS = 0, 1, 2
RANDOM_BYTES = (3, 7, 7, 7, 9, 200, 254, 255)
N_RANDOM = 16


def stamp(level, ring):
    return (level << 24) | ring


# ---- the reference ------------------------------------------------------------------------------------------------------------------

def fixpoint_pairs(img, t0, max_level):
    """The fixpoint as two int64 planes (level, ring); never coloured: level 255, ring 0.  Rings are unbounded."""
    img = np.asarray(img)
    h, w = img.shape
    n = h * w
    byte = img.reshape(-1).tolist()
    takes = np.zeros((h, w), dtype=bool)
    if h >= 3 and w >= 3:
        takes[1:-1, 1:-1] = img[1:-1, 1:-1] <= max_level      # border pixels never change; a level above the maximum never opens
    takes = takes.reshape(-1).tolist()
    inf = (255, 0)
    held = []
    for v in np.asarray(t0, dtype=np.uint32).reshape(-1).tolist():
        assert v <= KEY_INF, hex(v)
        held.append(inf if v == KEY_INF else (v >> 24, v & RING_MASK))
    heap = [(k, p) for p, k in enumerate(held) if k != inf]
    heapq.heapify(heap)
    while heap:
        k, p = heapq.heappop(heap)
        if k != held[p]:
            continue                                   # a stale entry: the pixel has fallen since
        lev, ring = k
        # (p - 1 of a pixel in column 0 and p + 1 of one in column w - 1 are border pixels of the neighbouring row: they take nothing)
        for q in (p - w, p + w, p - 1, p + 1):
            if q < 0 or q >= n or not takes[q]:
                continue
            offer = (byte[q], 1) if byte[q] > lev else (lev, ring + 1)
            if offer < held[q]:
                held[q] = offer
                heapq.heappush(heap, (offer, q))
    levels = np.array([k[0] for k in held], dtype=np.int64).reshape(h, w)
    rings = np.array([k[1] for k in held], dtype=np.int64).reshape(h, w)
    return levels, rings


def beyond_contract(levels, rings):
    """The pixels whose finite stamp holds a ring the contract refuses."""
    return (levels < 255) & (rings > LAST_RING)


def pack(levels, rings):
    """(level << 24) + ring in 32 bits, as the device's addition leaves it (a ring past the field carries into the level)."""
    return np.where(levels == 255, KEY_INF, ((levels << 24) + rings) & 0xFFFFFFFF).astype(np.uint32)


def planted_fixpoint(img, t0, max_level):
    """-> (packed u32 plane, overflow).  The plane is meaningful only when overflow is False."""
    levels, rings = fixpoint_pairs(img, t0, max_level)
    return pack(levels, rings), bool(beyond_contract(levels, rings).any())


# ---- corridors ----------------------------------------------------------------------------------------------------------------------

def _run_length(line, start, step, level, max_level):
    """Pixels a flood of `level` reaches from the border pixel `start` of a corridor before a wall or a higher level stops it."""
    n, x = 0, start + step
    while 0 < x < len(line) - 1 and line[x] <= max_level and line[x] <= level:
        n += 1
        x += step
    return n


def _corridors(n_lines, length, residues, modulus, level, max_level, top, raised):
    """`n_lines` rows of `length` pixels, corridors along the odd rows.  -> img, t0, facts (one dict per corridor).
    top: every source's ring is LAST_RING minus the length of its run; raised: index of the corridor whose first source gets
    one ring more than that (None: no corridor)."""
    assert length >= modulus + 5 and n_lines >= 3
    img = np.full((n_lines, length), 255, dtype=np.uint8)
    t0 = np.full((n_lines, length), KEY_INF, dtype=np.uint32)
    facts = []
    for k in range((n_lines - 1) // 2):
        y, direction, j = 2 * k + 1, k % 2, k // 2          # direction 0: fed from column 0; j: index among its direction's corridors
        kind = j % 3
        x = residues[j % len(residues)] + modulus * ((j + j // 3) % 3)
        while x < 2:
            x += modulus
        while x > length - 3:
            x -= modulus
        assert 2 <= x <= length - 3
        blocker = BLOCKER_LEVELS[(j // 3) % 3] if kind == KIND_LEVEL else 255
        img[y, 1:-1] = level
        img[y, x] = blocker
        line = img[y].tolist()
        near, far = (0, length - 1) if direction == 0 else (length - 1, 0)
        step = 1 if direction == 0 else -1
        sources = [(near, step, 1 + (7 * k) % 97)]
        if kind == KIND_WALL_TWO_FRONTS:
            sources.append((far, -step, 1 + (11 * k) % 89))
        placed = []
        for i, (sx, sstep, ring) in enumerate(sources):
            if top:
                ring = LAST_RING - _run_length(line, sx, sstep, level, max_level) + (1 if raised == k and i == 0 else 0)
            assert ring >= 1
            t0[y, sx] = stamp(level, ring)
            placed.append((sx, sstep, ring))
        facts.append({"line": y, "direction": direction, "kind": kind, "blocker_at": x, "blocker": blocker, "level": level,
                      "sources": placed})
    return img, t0, facts


def corridor_closed_form(line, level, sources, max_level):
    """One corridor by hand: every source's flood walked along the line, the smaller stamp wins.  -> list of (level, ring)."""
    out = [(255, 0)] * len(line)
    for sx, step, ring in sources:
        out[sx] = (level, ring)
    for sx, step, ring in sources:
        cur = (level, ring)
        x = sx + step
        while 0 < x < len(line) - 1 and line[x] <= max_level:
            cur = (line[x], 1) if line[x] > cur[0] else (cur[0], cur[1] + 1)
            out[x] = min(out[x], cur)
            x += step
    return out


@functools.lru_cache(maxsize=None)
def _corridor_case(family, w, h, level, max_level, top, raised):
    if family == "rows":
        img, t0, facts = _corridors(h, w, LANE_RESIDUES, 256, level, max_level, top, raised)
    else:
        img, t0, facts = _corridors(w, h, BAND_RESIDUES, 64, level, max_level, top, raised)
        img, t0 = np.ascontiguousarray(img.T), np.ascontiguousarray(t0.T)
    img.setflags(write=False)
    t0.setflags(write=False)
    return img, t0, facts


ROWS_SHAPE, ROWS_SCALAR_SHAPE, COLUMNS_SHAPE = (776, 131), (774, 131), (260, 200)      # (W, H)
HIGH_LEVELS = ((7, 254), (253, 253), (254, 254))      # (corridor level, max_level)
# the corridor whose source a twin raises: one fed from each side, its far end deep inside the plane
TWIN_CORRIDOR = {"rows": 21, "columns": 40}


def rows(w=ROWS_SHAPE[0], h=ROWS_SHAPE[1], level=7, max_level=254, top=False, raised=None, with_facts=False):
    img, t0, facts = _corridor_case("rows", w, h, level, max_level, top, raised)
    return (img, t0, max_level, facts) if with_facts else (img, t0, max_level)


def columns(w=COLUMNS_SHAPE[0], h=COLUMNS_SHAPE[1], level=7, max_level=254, top=False, raised=None, with_facts=False):
    img, t0, facts = _corridor_case("columns", w, h, level, max_level, top, raised)
    return (img, t0, max_level, facts) if with_facts else (img, t0, max_level)


def high_rings(family, level, with_facts=False):
    max_level = dict(HIGH_LEVELS)[level]
    return (rows if family == "rows" else columns)(level=level, max_level=max_level, top=True, with_facts=with_facts)


def overflow_twin(family, level, with_facts=False):
    max_level = dict(HIGH_LEVELS)[level]
    return (rows if family == "rows" else columns)(level=level, max_level=max_level, top=True, raised=TWIN_CORRIDOR[family],
                                                   with_facts=with_facts)


# ---- random upper bounds --------------------------------------------------------------------------------------------------------------

RANDOM_CORNERS = ((33, 250), (70, 528), (70, 530), (33, 252))      # the ends of both ranges, in both W % 4 classes


@functools.lru_cache(maxsize=None)
def random_case(i):
    rng = np.random.default_rng(7100 + i)
    if i < len(RANDOM_CORNERS):
        h, w = RANDOM_CORNERS[i]
    else:
        h, w = int(rng.integers(33, 71)), int(rng.integers(250, 531))
        if i % 2:                     # odd cases: W % 4 == 0
            w -= w % 4
            w = max(w, 252)
        elif w % 4 == 0:
            w += (1 + i % 3) if w + 3 <= 530 else -(1 + i % 3)
    max_level = 254 if (i // 2) % 2 == 0 else 100
    img = np.array(RANDOM_BYTES, dtype=np.uint8)[rng.integers(0, len(RANDOM_BYTES), (h, w))]
    u = rng.random((h, w))
    high = min(0xFFF000, (1 << 24) - 2 - h * w)
    rings = np.array([1, 2, 100, high], dtype=np.uint32)[rng.integers(0, 4, (h, w))]
    levels = rng.integers(0, 255, (h, w)).astype(np.uint32)
    t0 = np.full((h, w), KEY_INF, dtype=np.uint32)
    planted = u < 0.15
    t0[planted] = (levels[planted] << 24) | rings[planted]
    t0[(u >= 0.15) & (u < 0.17)] = 0
    img.setflags(write=False)
    t0.setflags(write=False)
    return img, t0, max_level


# ---- the list the tests share -----------------------------------------------------------------------------------------------------------

def _cases():
    out = {"rows/776": lambda: rows(), "rows/774": lambda: rows(w=ROWS_SCALAR_SHAPE[0]), "columns/260": lambda: columns()}
    for family in ("rows", "columns"):
        for level, _ in HIGH_LEVELS:
            out[f"high/{family}/{level}"] = functools.partial(high_rings, family, level)
            out[f"twin/{family}/{level}"] = functools.partial(overflow_twin, family, level)
    for i in range(N_RANDOM):
        out[f"random/{i:02d}"] = functools.partial(random_case, i)
    return out


CASES = _cases()
SOUND = tuple(n for n in CASES if not n.startswith("twin/"))      # every case the library must relax without complaint
TWINS = tuple(n for n in CASES if n.startswith("twin/"))


@functools.lru_cache(maxsize=None)
def reference(name):
    """planted_fixpoint of a named case, computed once (read-only)."""
    img, t0, max_level = CASES[name]()
    plane, overflow = planted_fixpoint(img, t0, max_level)
    plane.setflags(write=False)
    return plane, overflow
