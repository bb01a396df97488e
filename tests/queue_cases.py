"""Corridors flooded from seeds in the geometry of the tile queue (k_relax, PERSIST): 128 x 128 tiles, 32 bands, half rows of 32 lanes.

The planted planes of tests/planted_cases.py reach the kernels behind ws_block_relax.  The queue kernels take a seed plane and a
persist_mode, so these cases are whole transforms: (img, seeds, max_level), the seed list strictly increasing in row-major order
(the seed-table form), every seed on an interior pixel (a border seed never floods), W % 4 == 0 (relax_plan offers the queue to
no other width).  Blocker kinds, blocker levels and the closed form of one corridor are planted_cases': KIND_*, BLOCKER_LEVELS,
HIGH_LEVELS, corridor_closed_form -- a seed is a source of level 0 and ring 0.  Inputs of tests/test_gpu_queue_corridors.py;
tests/test_queue_cases_cpu.py proves on the CPU that every family reaches what it claims.

Families (every generator is deterministic):
  rows        walls of 255 with one-pixel corridors of level 7 on every second row, a seed on the first interior pixel at the left
              or, alternately, the right end, one blocker each: a higher level (9, 200, 254), a wall, or a wall with a second seed
              at the far end (two fronts).  Per direction the blocker columns cover every residue x mod 128 of LANE_RESIDUES --
              lanes 0, 15, 16 and 31 times the four patch columns: the DPP row ends, the row_bcast:15 hand-over and both ends of
              a half row of the SPLIT kernels -- with every kind at every residue, ROWS_LEAD = 1024 columns or more from the seed
              that feeds them.  1416 x 193: the last 128-column tile is 8 columns wide, the plane spans two 128-row tiles.
  columns     the transpose: corridors on every second column, fed from the top or the bottom, blocker rows covering every
              residue y mod 128 per direction -- every patch row of all 32 bands of a 128-row tile, its first and last rows among
              them --, every kind in every band, COLUMNS_LEAD = 512 rows or more from the seed.  516 x 650: the last 128-column
              tile is one patch column wide.
  serpentine  ONE seed and one single path: legs on every second row, joined alternately at the right and the left end, 520 x 151
              (75 legs, two 128-row tiles, a last tile column of 8).  32 level blockers, each one level higher than the one
              before along the path (8 .. 39), at every residue of LANE_RESIDUES in both directions; max_level 60, so that the
              flood-order buckets hold two levels each and the path climbs through 17 of them.  Every hop is a hand-off of the
              queue, 301 tile hops in all (tile_hops).
  twins       rows at (253, 253) and (254, 254) of planted_cases.HIGH_LEVELS (the top bucket, the other patch_bases path), and
              at level 7 with max_level 20 (one level per bucket; the 200 and 254 blockers are never flooded).
  stack       three slices of rows 67 high and two 131 high: slice walls at rows 67, 134 and 131, inside a 128-row queue tile.
"""
import functools

import numpy as np

import planted_cases as pc

QT = 128                                                                                  # the queue's tile: QT x QT pixels
LANE_RESIDUES = tuple(4 * lane + c for lane in (0, 15, 16, 31) for c in range(4))      # x mod 128
BAND_RESIDUES = tuple(range(QT))                                                          # y mod 128
ROWS_LEAD, COLUMNS_LEAD = 1024, 512
ROWS_SHAPE, COLUMNS_SHAPE, SERPENTINE_SHAPE = (1416, 193), (516, 650), (520, 151)      # (W, H)
ROWS_SCALAR_WIDTH = ROWS_SHAPE[0] - 2                                                     # the general-form twin: W % 4 != 0
SERPENTINE_MAX_LEVEL = 60
STACKS = ((3, 67), (2, 131))                                                              # (slices, slice height)
LEVEL = 7


def relax_tiles(h, w):
    """relax_plan_tiles (ws_relax_plan.hpp): run_fused_form picks the queue by itself for 1 .. relax_tiles / 2 seeds."""
    return max(((w + 255) // 256 + 1) * ((h + 31) // 32 + 1), ((w + 127) // 128 + 1) * ((h + 63) // 64 + 1))


def _rows_kind(j):
    return (j + j // len(LANE_RESIDUES)) % 3      # j, j + 16, j + 32 hold the same residue: the three kinds


def _columns_kind(j):
    return (j % 4 + j // 4) % 3                   # the four rows of a band: all three kinds


def _corridors(n_lines, length, residues, lead, kind_of, level, max_level, shift):
    """`n_lines` rows of `length` pixels, corridors along the odd rows.  -> img, seeds (line, position), facts (one dict per
    corridor: sources are corridor_closed_form's, (position, step, ring 0))."""
    assert n_lines >= 3 and length - 3 - (1 + lead) >= QT - 1      # every residue fits behind the lead
    img = np.full((n_lines, length), 255, dtype=np.uint8)
    seeds, facts = [], []
    n_levels = [0, 0]                                           # level blockers so far, per direction: their levels take turns
    for k in range((n_lines - 1) // 2):
        y, direction, j = 2 * k + 1, k % 2, k // 2 + shift      # direction 0: fed from column 1; j: index among its direction's
        kind = kind_of(j)
        near, far, step = (1, length - 2, 1) if direction == 0 else (length - 2, 1, -1)
        lo, hi = (near + lead, length - 3) if direction == 0 else (2, near - lead)
        residue = residues[j % len(residues)]
        fits = [x for x in range(residue, length, QT) if lo <= x <= hi]
        x = fits[(j + j // len(residues)) % len(fits)]
        blocker = 255
        if kind == pc.KIND_LEVEL:
            blocker = pc.BLOCKER_LEVELS[n_levels[direction] % 3]
            n_levels[direction] += 1
        img[y, 1:-1] = level
        img[y, x] = blocker
        sources = [(near, step, 0)]
        if kind == pc.KIND_WALL_TWO_FRONTS:
            sources.append((far, -step, 0))
        seeds += [(y, sx) for sx, _, _ in sources]
        facts.append({"line": y, "direction": direction, "kind": kind, "blocker_at": x, "blocker": blocker, "level": level,
                      "sources": sources})
    return img, seeds, facts


def _seed_array(seeds):
    out = np.array(sorted(seeds), dtype=np.uint64).reshape(-1, 2)      # row-major order
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _corridor_case(family, w, h, level, max_level, shift):
    if family == "rows":
        img, seeds, facts = _corridors(h, w, LANE_RESIDUES, ROWS_LEAD, _rows_kind, level, max_level, shift)
    else:
        img, seeds, facts = _corridors(w, h, BAND_RESIDUES, COLUMNS_LEAD, _columns_kind, level, max_level, shift)
        img, seeds = np.ascontiguousarray(img.T), [(x, y) for y, x in seeds]
    img.setflags(write=False)
    return img, _seed_array(seeds), facts


def rows(w=ROWS_SHAPE[0], h=ROWS_SHAPE[1], level=LEVEL, max_level=254, shift=0, with_facts=False):
    img, seeds, facts = _corridor_case("rows", w, h, level, max_level, shift)
    return (img, seeds, max_level, facts) if with_facts else (img, seeds, max_level)


def columns(w=COLUMNS_SHAPE[0], h=COLUMNS_SHAPE[1], level=LEVEL, max_level=254, shift=0, with_facts=False):
    img, seeds, facts = _corridor_case("columns", w, h, level, max_level, shift)
    return (img, seeds, max_level, facts) if with_facts else (img, seeds, max_level)


# ---- the serpentine -----------------------------------------------------------------------------------------------------------------

def _spread(n, of):
    """n of the indices 0 .. of - 1, the first and the last among them."""
    return [round(i * (of - 1) / (n - 1)) for i in range(n)]


@functools.lru_cache(maxsize=None)
def _serpentine(w, h):
    img = np.full((h, w), 255, dtype=np.uint8)
    n_legs = (h - 1) // 2
    path = []
    for k in range(n_legs):
        y = 2 * k + 1
        xs = range(1, w - 1) if k % 2 == 0 else range(w - 2, 0, -1)      # even legs run to the right
        path += [(y, x) for x in xs]
        if k + 1 < n_legs:
            path.append((y + 1, w - 2 if k % 2 == 0 else 1))             # the joint to the next leg
    ys, xs = (np.array(v) for v in zip(*path))
    img[ys, xs] = LEVEL
    # 16 legs of each direction hold one blocker, spread over the path's whole length (both tile rows)
    per = len(LANE_RESIDUES)
    chosen = [(2 * i, 0, n) for n, i in enumerate(_spread(per, (n_legs + 1) // 2))]
    chosen += [(2 * i + 1, 1, n) for n, i in enumerate(_spread(per, n_legs // 2))]
    blockers = []
    for k, direction, n in sorted(chosen):                               # in path order: each one level higher
        fits = [x for x in range(LANE_RESIDUES[n], w, QT) if 3 <= x <= w - 4]
        x = fits[(n + n // 4 + direction) % len(fits)]
        level = LEVEL + 1 + len(blockers)
        img[2 * k + 1, x] = level
        blockers.append({"leg": k, "direction": direction, "blocker_at": x, "blocker": level})
    img.setflags(write=False)
    return img, _seed_array([path[0]]), tuple(path), blockers


def serpentine(w=SERPENTINE_SHAPE[0], h=SERPENTINE_SHAPE[1], with_facts=False):
    img, seeds, path, blockers = _serpentine(w, h)
    return (img, seeds, SERPENTINE_MAX_LEVEL, path, blockers) if with_facts else (img, seeds, SERPENTINE_MAX_LEVEL)


def tile_hops(path):
    """How often the path enters another tile of the queue's grid."""
    tiles = [(y // QT, x // QT) for y, x in path]
    return sum(a != b for a, b in zip(tiles, tiles[1:]))


# ---- stacks of slices -----------------------------------------------------------------------------------------------------------------

def stack(slices, slice_h):
    """-> (cube (S, H, W) uint8, list of per-slice seed arrays, max_level): rows of slice_h lines, each slice with its own
    blocker positions (shift)."""
    parts = [rows(h=slice_h, shift=5 * s) for s in range(slices)]
    cube = np.stack([p[0] for p in parts])
    cube.setflags(write=False)
    return cube, [p[1] for p in parts], 254


# ---- the list the tests share -----------------------------------------------------------------------------------------------------------

SCALAR_TWIN = "rows/1414"                                                   # not in CASES: no queue at this width
ROWS_FORMS = {"rows/1416": {}, "rows/max20": {"max_level": 20}, SCALAR_TWIN: {"w": ROWS_SCALAR_WIDTH}}      # name -> arguments of rows()
ROWS_FORMS.update({f"rows/level{level}": {"level": level, "max_level": max_level} for level, max_level in pc.HIGH_LEVELS[1:]})


def _cases():
    out = {"columns/516": columns, "serpentine/520": serpentine}
    out.update({name: functools.partial(rows, **kw) for name, kw in ROWS_FORMS.items() if name != SCALAR_TWIN})
    return out


CASES = _cases()
CORRIDORS = tuple(n for n in CASES if not n.startswith("serpentine/"))      # many seeds: the default gives the early schedule


def scalar_twin():
    return rows(**ROWS_FORMS[SCALAR_TWIN])
