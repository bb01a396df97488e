"""Inputs that put the 2-D tiled transforms (tiled2d_rank in csrc/ws_tiled.hip: column packing, the ring resolve, the "no received
ring differs" test, the padded pair table) where they go wrong and where the row-block families of tests/tiled_cases.py never
look: column seams, tiles of one or two columns, the pixels where a row seam meets a column seam, corridors that wind across
column seams and around the crossing point, plateaus whose ties fall on seams, lakes joined only through other tiles.  Plain
numpy, seeded by name, no GPU.  tests/test_tiled2d_cases_cpu.py proves on the oracle that every family reaches its regime (and
runs the protocol on the numpy stand-in over gloo); tests/test_gpu_tiled2d_edges.py compares the HIP kernels with the oracle bit
for bit.

Every case is (name, image, seeds, grids): `grids` lists the (py, px) the case is meant for, py * px <= 8 always.  Families:

  t  the row families a to f of tiled_cases transposed, on (1, world) -- and the originals of a, b, d, e on (world, 1), which
     takes them through tiled2d_rank (painted seeds, ring resolve) where tiled_cases runs them through the row-block program
  u  thin tiles: every tile owns one or two columns (rows), held planes 2 and 3 wide; and two splits that do not divide
  v  seeds on the 2 x 2 quads where a row seam meets a column seam, on whole seam columns, on the field's border next to seams
  w  corridors one pixel wide: a horizontal serpentine (40 crossings of every column seam), spirals round the crossing point
  x  a constant plane: ring counts are Manhattan distances, ties between parents on either side of a seam
  y  lakes whose pieces inside a tile are joined only through other tiles
  z  edge correction through the host call, down to a tile that owns only the virtual ring column

Side tables, by case name: merge_levels(name), W_PATH / corridor_K (family w), V_SPECIAL (family v), Y_META (family y).
"""
import numpy as np

import tiled_cases as tc


# ---- the cut: Group.tile_grid / tile_split (csrc/ws_tile_plan.hpp), restated ----------------------------------------------------

def tile_grid(h, w, rank, py, px):
    """((r0, r1, lo, hi), (c0, c1, clo, chi)) of rank = ty * px + tx: ws_tile_grid.  A split that does not divide gives the extra
    line to the first parts."""
    assert py >= 1 and px >= 1 and 0 <= rank < py * px
    return tc.tile_rows(h, rank // px, py), tc.tile_rows(w, rank % px, px)


def tiles(h, w, py, px):
    return [tile_grid(h, w, k, py, px) for k in range(py * px)]


def seam_starts(n, parts):
    """The first owned line of parts 1 .. parts - 1: line s - 1 and line s lie on either side of a seam."""
    return [tc.tile_rows(n, k, parts)[0] for k in range(1, parts)]


def owner(h, w, py, px, r, c):
    """The rank that owns pixel (r, c)."""
    ty = sum(1 for s in seam_starts(h, py) if r >= s)
    tx = sum(1 for s in seam_starts(w, px) if c >= s)
    return ty * px + tx


def owner_plane(h, w, py, px):
    out = np.zeros((h, w), dtype=np.int64)
    for k, ((r0, r1, _, _), (c0, c1, _, _)) in enumerate(tiles(h, w, py, px)):
        out[r0:r1, c0:c1] = k
    return out


def _shuffled(name, s):
    p = s[tc._rng(name + "/shuffled").permutation(len(s))]
    if len(s) >= 2 and (p == s).all():
        p = s[::-1].copy()
    return p


# ---- t: the row families transposed, and the originals through tiled2d_rank -------------------------------------------------------

def transposed_rows():
    """(tiled_cases' own oracle results do not carry over: the parent order D, R, L, U is not symmetric under transposition.)"""
    out = []
    for name, img, seeds, world in tc.all_cases("abcdef"):
        s = np.asarray(seeds, dtype=np.int64).reshape(-1, 2)
        st = np.ascontiguousarray(s[:, ::-1])
        if tc.is_strictly_increasing(s, img.shape[1]):      # a sorted list stays a sorted list
            st = tc._sorted(st)
        out.append((f"t/T/{name}", np.ascontiguousarray(img.T), st, [(1, world)]))
        if name[0] in "abde":
            out.append((f"t/O/{name}", img, s.copy(), [(world, 1)]))
    return out


# ---- u: thin tiles ----------------------------------------------------------------------------------------------------------------

THIN_PARTS = (2, 3, 4, 8)
THIN_LENGTHS = (4, 33, 260)
THIN_GRIDS = ((2, 2), (2, 3), (3, 2), (2, 4), (4, 2))
UNEVEN = ((7, 11, (2, 3)), (13, 9, (3, 2)))


def thin_tiles():
    """u/cols*: h x px and h x 2 px on (1, px); u/rows*: the same with rows and columns swapped on (py, 1); u/grid*: py x px and
    2 py x 2 px; u/uneven: tiles of unequal size (the pair table is padded to the largest).  Every second list is shuffled."""
    out = []

    def case(tag, h, w, grid):
        name = f"u/{tag}/{h}x{w}"
        rng = tc._rng(name)
        img = tc._noise(rng, h, w)
        s = tc._sorted(tc._random_seeds(rng, h, w, max(2, h * w // 6)))
        out.append((name, img, _shuffled(name, s) if len(out) % 2 else s, [grid]))

    for p in THIN_PARTS:
        for n in THIN_LENGTHS:
            case(f"cols{p}", n, p, (1, p))
            case(f"cols{p}", n, 2 * p, (1, p))
            case(f"rows{p}", p, n, (p, 1))
            case(f"rows{p}", 2 * p, n, (p, 1))
    for py, px in THIN_GRIDS:
        case(f"grid{py}x{px}", py, px, (py, px))
        case(f"grid{py}x{px}", 2 * py, 2 * px, (py, px))
    for h, w, grid in UNEVEN:
        case("uneven", h, w, grid)
    return out


# ---- v: seeds on crossings --------------------------------------------------------------------------------------------------------

CROSS_SHAPE = (40, 48)
CROSS_GRIDS = ((2, 2), (2, 3), (3, 2))
V_SPECIAL = {}      # name -> (kind, grid, the pixels the case is about, index of the doubled entry's first occurrence or None)


def quad(h, w, py, px, i, j):
    """The four pixels where row seam i meets column seam j (0-based), row-major."""
    rs, cs = seam_starts(h, py)[i], seam_starts(w, px)[j]
    return [(rs - 1, cs - 1), (rs - 1, cs), (rs, cs - 1), (rs, cs)]


def crossing_seeds():
    """Every case: the pixels it is about plus six seeds elsewhere (so that floods compete for the pixels around them), as a
    sorted list, shuffled, and with one of the special pixels a second time at the end (/dup: the later entry's colour wins)."""
    h, w = CROSS_SHAPE
    img = tc._noise(tc._rng("v/field"), h, w)
    out = []

    def case(name, grid, kind, special):
        special = [tuple(int(v) for v in p) for p in special]
        rng = tc._rng(name)
        extra = [tuple(int(v) for v in p) for p in tc._random_seeds(rng, h, w, 6)]
        s = tc._sorted(special + [p for p in extra if p not in set(special)])
        k = int(np.flatnonzero((s == np.array(special[len(special) // 2])).all(axis=1))[0])
        for form, lst in (("sorted", s), ("shuffled", _shuffled(name, s)), ("dup", np.concatenate([s, s[k][None, :]]))):
            out.append((f"{name}/{form}", img, lst, [grid]))
            V_SPECIAL[f"{name}/{form}"] = (kind, grid, special, k if form == "dup" else None)

    for py, px in CROSS_GRIDS:
        g = f"g{py}x{px}"
        rows, cols = seam_starts(h, py), seam_starts(w, px)
        for i in range(py - 1):
            for j in range(px - 1):
                q = quad(h, w, py, px, i, j)
                case(f"v/{g}/quad{i}{j}", (py, px), ("quad", i, j), q)
                for n, p in enumerate(q):
                    case(f"v/{g}/quad{i}{j}/alone{n}", (py, px), ("alone", i, j, n), [p])
        case(f"v/{g}/seam_columns", (py, px), ("columns",), [(r, c) for r in range(h) for cs in cols for c in (cs - 1, cs)])
        border = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
        border += [(r, c) for cs in cols for c in (cs - 1, cs) for r in (0, h - 1)]
        border += [(r, c) for rs in rows for r in (rs - 1, rs) for c in (0, w - 1)]
        case(f"v/{g}/border", (py, px), ("border",), border)
    return out


# ---- w: corridors -----------------------------------------------------------------------------------------------------------------

CORRIDOR_LEVEL = 4
W_PATH = {}      # name -> the corridor's pixels from the seed to its far end, in order


def walk(img, start):
    """The unique path through the open pixels (< 255) from `start`; asserts that it never forks."""
    h, w = img.shape
    path, prev = [tuple(start)], None
    while True:
        r, c = path[-1]
        nxt = [(y, x) for y, x in ((r + 1, c), (r, c + 1), (r, c - 1), (r - 1, c))
               if 0 <= y < h and 0 <= x < w and img[y, x] < 255 and (y, x) != prev]
        assert len(nxt) <= 1, (r, c, nxt)
        if not nxt:
            return path
        prev = path[-1]
        path.append(nxt[0])


def crossings(path, shape, grid):
    """The seams a path crosses, in order: "row" or "col" for every step between pixels of different tiles."""
    own = owner_plane(*shape, *grid)
    out = []
    for (r, c), (y, x) in zip(path[:-1], path[1:]):
        if own[r, c] != own[y, x]:
            out.append("row" if y != r else "col")
    return out


def corridor_K(name, grid):
    """Seam crossings on the corridor's path from the seed to its far end."""
    img = BY_NAME[name][1]
    return len(crossings(W_PATH[name], img.shape, grid))


def spiral(h, w):
    """Walls of 255, a corridor of pitch 2 that starts at (1, 1) and winds clockwise inwards round the crossing point of a
    (2, 2) cut (h and w even): right along the top, down the right, left along the bottom, up the left.  It ends before the
    first arm that would not cross its seam, so every arm crosses one: column, row, column, row ...  Returns (image, path)."""
    assert h % 2 == 0 and w % 2 == 0
    rs, cs = h // 2, w // 2
    img = np.full((h, w), 255, dtype=np.uint8)
    top, bottom, left, right = 1, h - 2, 1, w - 2
    r, c = 1, 1
    path = [(1, 1)]
    while True:
        if not (c < cs <= right):
            break
        path += [(r, x) for x in range(c + 1, right + 1)]
        c = right
        top += 2
        if not (r < rs <= bottom):
            break
        path += [(y, c) for y in range(r + 1, bottom + 1)]
        r = bottom
        right -= 2
        if not (left < cs <= c):
            break
        path += [(r, x) for x in range(c - 1, left - 1, -1)]
        c = left
        bottom -= 2
        if not (top < rs <= r):
            break
        path += [(y, c) for y in range(r - 1, top - 1, -1)]
        r = top
        left += 2
    for y, x in path:
        img[y, x] = CORRIDOR_LEVEL
    return img, path


SPIRALS = ((30, 34, [(2, 2)]), (46, 50, [(2, 2)]), (70, 1100, [(1, 2), (2, 2)]))
SERPENTINE_GRIDS = [(1, 4), (1, 2)]


def corridors():
    out = []
    # (i) zigzag() of 82 columns has 40 vertical corridors; transposed, 40 horizontal ones of 128 pixels: 40 crossings of every
    # column seam
    img = np.ascontiguousarray(tc.zigzag(h=130, w=82).T)
    name = "w/serpentine/82x130"
    out.append((name, img, np.array([[1, 1]], dtype=np.int64), list(SERPENTINE_GRIDS)))
    W_PATH[name] = walk(img, (1, 1))
    # (ii), (iii)
    for h, w, grids in SPIRALS:
        img, path = spiral(h, w)
        name = f"w/spiral/{h}x{w}"
        out.append((name, img, np.array([[1, 1]], dtype=np.int64), list(grids)))
        W_PATH[name] = path
    return out


# ---- x: plateaus and ties ---------------------------------------------------------------------------------------------------------

PLATEAU_SHAPE = (33, 64)
PLATEAU_LEVEL = 9


def plateaus():
    """x/one: a seed on the crossing quad of the (2, 2) cut.  x/two: P = (rs - 7, cs - 7) and Q = (rs + 5, cs + 17), 12 rows and 24
    columns apart, rs and cs the first row and column after a seam.  The pixels equidistant from both are an antidiagonal inside
    the box the seeds span -- it meets row rs - 1, the last above the seam, where the D neighbour (first in D, R, L, U, in the
    tile below) is one ring nearer to Q -- and, below the box, column cs - 1, the last before the seam: there D is farther from
    both and the R neighbour, in the tile to the right, wins."""
    h, w = PLATEAU_SHAPE
    img = np.full((h, w), PLATEAU_LEVEL, dtype=np.uint8)
    out = [("x/one", img, np.array([[16, 31]], dtype=np.int64), [(2, 2), (1, 4), (2, 3)])]
    for tag, grids, cs in (("a", [(2, 2), (1, 4)], 32), ("b", [(2, 3)], seam_starts(w, 3)[0])):
        rs = seam_starts(h, 2)[0]
        s = np.array([[rs - 7, cs - 7], [rs + 5, cs + 17]], dtype=np.int64)
        out.append((f"x/two/{tag}/sorted", img, s, grids))
        out.append((f"x/two/{tag}/shuffled", img, s[::-1].copy(), grids))
    return out


# ---- y: lakes linked through other tiles ------------------------------------------------------------------------------------------

LINK_LEVEL = 40
BASIN_LEVEL = 3
Y_META = {}      # name -> (mask of the named lake, {grid: rank of the named tile}, link level)


def _forms(name, img, s, grids, mask, tile, link):
    s = tc._sorted(s)
    for form, lst in (("sorted", s), ("shuffled", s[::-1].copy())):
        Y_META[f"{name}/{form}"] = (mask, tile, link)
        yield (f"{name}/{form}", img, lst, grids)


def corner_link():
    """24 x 28 on (2, 2): seam rows 11 | 12, seam columns 13 | 14.  Basins in (0, 0) (two seeds) and (1, 1) (none), a corridor at
    LINK_LEVEL from the first along row 5 into (0, 1), down column 20 into the second; a finger of the second basin reaches up
    column 24 into (0, 1) without touching the corridor there; a basin with a seed of its own in (1, 0)."""
    img = np.full((24, 28), 255, dtype=np.uint8)
    img[2:9, 2:10] = BASIN_LEVEL
    img[5, 10:21] = LINK_LEVEL
    img[5:17, 20] = LINK_LEVEL
    img[17:22, 16:26] = BASIN_LEVEL
    img[9:17, 24] = BASIN_LEVEL
    mask = img < 255
    img[15:22, 2:10] = BASIN_LEVEL
    return img, np.array([[3, 3], [7, 8], [18, 5]], dtype=np.int64), mask


def round_trip():
    """24 x 28 on (2, 2): two basins in tile (0, 0), a seed in each, joined only by a corridor that leaves through the right seam
    (row 3), runs down column 20 into (1, 1), back along row 17 into (1, 0) and up column 5 through the bottom seam of (0, 0)."""
    img = np.full((24, 28), 255, dtype=np.uint8)
    img[2:5, 2:10] = BASIN_LEVEL
    img[7:10, 2:10] = BASIN_LEVEL
    img[3, 10:21] = LINK_LEVEL
    img[3:18, 20] = LINK_LEVEL
    img[17, 5:21] = LINK_LEVEL
    img[10:18, 5] = LINK_LEVEL
    return img, np.array([[3, 3], [8, 5]], dtype=np.int64), img < 255


def linked_through_tiles():
    out = []
    # (i) linked_field transposed: horizontal serpentines, joined at their ends in the first and last tile of (1, world)
    for h, w, world in tc.LINKED_SHAPES:
        src, left, right = tc.linked_field(h, w)
        img = np.ascontiguousarray(src.T)
        s = tc.linked_seeds(h, w, world, left, right)[:, ::-1]
        mask = np.zeros(img.shape, dtype=bool)
        mask[: w // 2] = img[: w // 2] < 255            # the upper lake (the source's left one)
        out += _forms(f"y/linked/{w}x{h}", img, s, [(1, world)], mask, {(1, world): 1}, int(img[mask].max()))
    img, s, mask = corner_link()
    out += _forms("y/corner", img, s, [(2, 2)], mask, {(2, 2): 1}, LINK_LEVEL)
    img, s, mask = round_trip()
    out += _forms("y/round_trip", img, s, [(2, 2)], mask, {(2, 2): 0}, LINK_LEVEL)
    return out


# ---- z: edge correction -----------------------------------------------------------------------------------------------------------

EDGE_SHAPES = ((2, 2, (2, 2)), (6, 6, (2, 2)), (6, 2, (2, 4)))


def edge_correction():
    """The padded plane is (h + 2) x (w + 2): 6 x 2 pads to 8 x 4, so on (2, 4) every tile owns one column and tile 0 only the
    virtual ring column.  /noshift/: the list names pixels of the padded plane; /shift/: pixels of the image, moved by the engine."""
    out = []
    for h, w, grid in EDGE_SHAPES:
        rng = tc._rng(f"z/{h}x{w}")
        img = tc._noise(rng, h, w)
        s = tc._sorted(tc._random_seeds(rng, h, w, max(2, h * w // 6)))
        for shift in (False, True):
            lst = s if shift else s + 1
            name = f"z/{h}x{w}/{'shift' if shift else 'noshift'}"
            out.append((name + "/sorted", img, lst, [grid]))
            out.append((name + "/shuffled", img, lst[::-1].copy(), [grid]))
    return out


# ---- all of them ------------------------------------------------------------------------------------------------------------------

FAMILIES = {"t": transposed_rows, "u": thin_tiles, "v": crossing_seeds, "w": corridors, "x": plateaus, "y": linked_through_tiles,
            "z": edge_correction}
_CACHE = {}
BY_NAME = {}


def family(letter):
    if letter not in _CACHE:
        _CACHE[letter] = FAMILIES[letter]()
        for c in _CACHE[letter]:
            assert c[0] not in BY_NAME and all(py * px <= 8 for py, px in c[3]), c[0]
            BY_NAME[c[0]] = c
    return _CACHE[letter]


def all_cases(letters="tuvwxyz"):
    return [c for l in letters for c in family(l)]


def merge_levels(name):
    """The levels a case is merged at."""
    f = name[0]
    if f == "t":
        return tc.LINKED_LEVELS if "/f/" in name else (254, 120, 60)
    if f == "w":
        return (254, CORRIDOR_LEVEL, CORRIDOR_LEVEL - 1)
    if f == "x":
        return (254, PLATEAU_LEVEL, PLATEAU_LEVEL - 1)
    if f == "y":      # the level at which the link floods, the level below it, and 254
        link = Y_META[name][2]
        return (link, link - 1, 254)
    return (254, 120, 60)


def pairs(letters="tuvwxyz"):
    """(case, (py, px)) for every grid of every case."""
    return [(c, g) for c in all_cases(letters) for g in c[3]]


def pair_id(case, grid):
    return f"{case[0]}@{grid[0]}x{grid[1]}"
