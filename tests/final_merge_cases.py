"""Inputs for the final merged labels of ws_merge_device (csrc/ws_merge_final.hip, union_image): the 64 x 64 "one-lake tile" route of
k_tile_scan, k_tile_links, k_tile_roots, k_union_seeds, k_tile_edges, k_union_tiles and k_relabel_tiles, which no other merging
entry point takes.  Plain numpy, seeded, no GPU, no oracle.  tests/test_final_merge_cases_cpu.py proves on the oracle that every
family is in its regime; tests/test_gpu_final_merge.py compares the device with the oracle bit for bit.

A case is (name, image, seeds, facts): seeds an (n, 2) int64 array of (row, col) as the caller passes them, facts a dict
  family     "D" (duplicate seed lists) or "L" (long runs of one-lake tiles)
  edge       edge correction: the plane (and the tile grid) is the image with a ring of zeros around it
  shift      ws_options.seed_shift: the engine moves the list one pixel in; without it the list indexes the padded plane as it is
  max_level  max_water_level
Family D adds
  entries    list positions i whose colour i + 1 is overwritten by a later entry on the same pixel and is meant to lie BELOW the id
             of the lake its pixel belongs to
  undercut   True: every one of `entries` lies in a one-lake tile ("one" cases) -- the tile whose root k_union_seeds would hook
             under a colour that exists nowhere.  False: overwritten, but on a corner (k_union_seeds skips it).  None: no claim
             (partial water levels: the tiles do not fill)
  twin       "one", or "general": the same image with one interior pixel of every entry's tile set to NEVER_FILL, so that the
             tile takes k_union_tiles; the same id rule must hold
  where      "interior", "border" or "corner": where the entries' pixels lie in the plane
Family L adds
  pattern    the tile classes, one string per tile row: O open (9), X NEVER_FILL with a cross of corridors, W NEVER_FILL throughout

plane_seeds(case) gives the list in the coordinates of the plane; classify() restates k_tile_scan on numpy.
"""
import zlib

import numpy as np

UT = 64                 # tile side of union_image
WAVE = 64               # consecutive tiles, in linear order, that k_tile_links scans together
NEVER_FILL = 255
KINDS = ("noise", "plateau", "flat")
D_SHAPES = ((3, 3), (64, 64), (66, 66), (65, 129), (72, 136), (67, 131))


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- the tile classification of k_tile_scan, on numpy ------------------------------------------------------------------------------

def interior_mask(shape):
    m = np.zeros(shape, dtype=bool)
    m[1:-1, 1:-1] = True
    return m


def is_corner(r, c, shape):
    return (r in (0, shape[0] - 1)) and (c in (0, shape[1] - 1))


def tile_of(r, c):
    return int(r) // UT, int(c) // UT


def classify(seg):
    """tile_min (tilesY, tilesX) of the segmenting label plane `seg`: 0 for a general tile; for a one-lake tile -- it holds an
    image-interior pixel and every image-interior pixel of it is coloured -- the smallest colour on its non-corner pixels."""
    seg = np.asarray(seg)
    h, w = seg.shape
    ty, tx = (h + UT - 1) // UT, (w + UT - 1) // UT
    inner = interior_mask(seg.shape)
    corner = np.zeros(seg.shape, dtype=bool)
    corner[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    out = np.zeros((ty, tx), dtype=np.uint64)
    for y in range(ty):
        for x in range(tx):
            sl = (slice(y * UT, (y + 1) * UT), slice(x * UT, (x + 1) * UT))
            s, i = seg[sl], inner[sl]
            if not i.any() or (s[i] == 0).any():
                continue
            out[y, x] = s[(s != 0) & ~corner[sl]].min()
    return out


def runs(tile_min):
    """The runs of one-lake tiles along the tile rows: dicts of ty, x0, x1 (inclusive), t0 (linear index of the head), lane0,
    mins (the tiles' tile_min) and crosses (linear indices t > t0 of the run with t % 64 == 0: a wave starts inside the run)."""
    ty, tx = tile_min.shape
    out = []
    for y in range(ty):
        x = 0
        while x < tx:
            if tile_min[y, x] == 0:
                x += 1
                continue
            x0 = x
            while x < tx and tile_min[y, x] != 0:
                x += 1
            t0 = y * tx + x0
            out.append({"ty": y, "x0": x0, "x1": x - 1, "t0": t0, "lane0": t0 % WAVE, "mins": tile_min[y, x0:x].copy(),
                        "crosses": [t for t in range(t0 + 1, y * tx + x) if t % WAVE == 0]})
    return out


def plane_shape(case):
    _, img, _, facts = case
    e = 2 if facts["edge"] else 0
    return img.shape[0] + e, img.shape[1] + e


def plane_seeds(case):
    """The list in the coordinates of the plane the transform works on (what the oracle takes)."""
    _, _, seeds, facts = case
    return seeds + (1 if facts["edge"] and facts["shift"] else 0)


# ---- images ------------------------------------------------------------------------------------------------------------------------

def image(kind, h, w, rng):
    if kind == "noise":
        return rng.integers(0, 254, (h, w), dtype=np.uint8)
    if kind == "plateau":      # four values: long ties, arrival rings in every direction
        return (rng.integers(0, 4, (h, w)) * 60).astype(np.uint8)
    if kind == "flat":
        return np.full((h, w), 9, dtype=np.uint8)
    raise ValueError(kind)


def _draw_interior(rng, shape, k, taken=()):
    """k distinct interior pixels of the plane (fewer where it has fewer), none of `taken`, row-major."""
    h, w = shape
    px = [(r, c) for r in range(1, h - 1) for c in range(1, w - 1) if (r, c) not in taken]
    if len(px) > k:
        px = [px[i] for i in sorted(rng.choice(len(px), size=k, replace=False))]
    return px


def _free_pixel(shape, tile, seed_set):
    """The first interior pixel of the tile, row-major, that holds no seed; None where there is none."""
    h, w = shape
    for r in range(max(tile[0] * UT, 1), min(tile[0] * UT + UT, h - 1)):
        for c in range(max(tile[1] * UT, 1), min(tile[1] * UT + UT, w - 1)):
            if (r, c) not in seed_set:
                return r, c
    return None


def _emit(out, name, img, pseeds, entries, where, undercut=True, edge=False, shift=False, max_level=254, twin=True):
    """The case and, where every entry's tile has a free interior pixel, its general twin.  pseeds: the list in plane coordinates."""
    pseeds = np.asarray(pseeds, dtype=np.int64).reshape(-1, 2)
    off = 1 if edge else 0
    seeds = np.ascontiguousarray(pseeds - (1 if edge and shift else 0))
    facts = {"family": "D", "edge": edge, "shift": shift, "max_level": max_level, "entries": list(entries), "undercut": undercut,
             "twin": "one", "where": where}
    out.append((name + "/one", img, seeds, facts))
    if not twin:
        return
    shape = (img.shape[0] + 2 * off, img.shape[1] + 2 * off)
    seed_set = {(int(r), int(c)) for r, c in pseeds}
    img2 = img.copy()
    for i in entries:
        p = _free_pixel(shape, tile_of(*pseeds[i]), seed_set)
        if p is None:
            return
        img2[p[0] - off, p[1] - off] = NEVER_FILL      # (an interior pixel of the plane is a pixel of the image)
    out.append((name + "/general", img2, seeds, dict(facts, twin="general")))


def _lists(shape, rng):
    """(tag, list in plane coordinates, entries, where, undercut) for one shape."""
    h, w = shape
    res = []
    if (h, w) == (3, 3):
        c = (1, 1)
        res.append(("centre_twice", [c, c], [0], "interior", True))                       # the smallest input there is
        res.append(("centre_thrice", [c, c, c], [0, 1], "interior", True))
        res.append(("border_top", [(0, 1), (0, 1)], [0], "border", True))                 # the centre floods from the border seed
        res.append(("border_left", [(1, 0), c, (1, 0)], [0], "border", True))
        for tag, p in (("corner_tl", (0, 0)), ("corner_tr", (0, 2)), ("corner_bl", (2, 0)), ("corner_br", (2, 2))):
            res.append((tag, [p, c, p], [0], "corner", False))
        return res
    base = _draw_interior(rng, shape, 12)
    k = len(base)
    res.append(("then_reversed", base + base[::-1], [0], "interior", True))               # colours k + 1 .. 2 k exist
    bl = (h - 2, 1)                                                                       # the last tile row: thin at 65, 66, 67, 72 rows
    rest = [p for p in base if p != bl]
    res.append(("thrice", [p for p in [bl] + rest for _ in range(3)], [0, 1], "interior", True))      # colours 3, 6, 9, ... exist
    res.append(("first_again", base + [base[0]], [0], "interior", True))                  # colour 1 is the overwritten one
    tr = (1, w - 2)                                                                       # the last tile column
    rest = [p for p in base if p != tr]
    tail = rest + [rest[i] for i in rng.choice(len(rest), size=5, replace=False)] + [tr]
    res.append(("shuffled", [tr] + [tail[i] for i in rng.permutation(len(tail))], [0], "interior", True))
    for tag, p in (("border_top", (0, w // 2)), ("border_bottom", (h - 1, w - 3)), ("border_left", (h // 2, 0)), ("border_right", (2, w - 1))):
        # (row 64 of 65 rows, column 128 of 129: the border pixel's tile has no interior pixel, is never one lake: no claim)
        res.append((tag, [p] + base[:6] + [p], [0], "border", True if _free_pixel(shape, tile_of(*p), ()) else None))
    for tag, p in (("corner_tl", (0, 0)), ("corner_tr", (0, w - 1)), ("corner_bl", (h - 1, 0)), ("corner_br", (h - 1, w - 1))):
        res.append((tag, [p] + base[:6] + [p], [0], "corner", False))
    assert k >= 7
    return res


_D = None


def d_cases():
    """Family D.  The image kind rotates through noise, plateau and flat, so that every list meets every kind on some shape."""
    global _D
    if _D is not None:
        return _D
    out = []
    n = 0
    for shape in D_SHAPES:
        h, w = shape
        rng = _rng(f"D/{h}x{w}")
        for tag, lst, entries, where, undercut in _lists(shape, rng):
            kind = KINDS[n % 3]
            n += 1
            _emit(out, f"D/{h}x{w}/{tag}/{kind}", image(kind, h, w, rng), lst, entries, where, undercut)
        n += 1      # (the lists of a shape are as many as the kinds times a whole number: shift the rotation)
    # two lakes, each of one-lake tiles, with a tile of NEVER_FILL between them; both hold an overwritten colour below their id
    for kind in KINDS:
        h, w = 64, 192
        rng = _rng(f"D/two_lakes/{kind}")
        img = image(kind, h, w, rng)
        img[:, 64:128] = NEVER_FILL
        a = [(r, c) for r, c in _draw_interior(rng, (h, 64), 5)]
        b = [(r, c + 128) for r, c in _draw_interior(rng, (h, 64), 5)]
        lst = [p for pair in zip(a, b) for p in pair] + [a[0], b[0]]      # colours 1 (lake a) and 2 (lake b) are overwritten
        _emit(out, f"D/two_lakes/64x192/{kind}", img, lst, [0, 1], "interior", True)
    # edge correction: the tile grid lies over the padded plane (66 x 66 and 67 x 131), the list is moved into it or not
    for (h, w) in ((64, 64), (65, 129)):
        for shift in (False, True):
            rng = _rng(f"D/edge/{h}x{w}/{shift}")
            for tag, lst, entries, where, undercut in _lists((h + 2, w + 2), rng):
                if tag not in ("then_reversed", "first_again", "border_left", "corner_br"):
                    continue
                if shift and where != "interior":
                    continue                     # (a list moved one pixel in never names the ring)
                kind = KINDS[n % 3]
                n += 1
                _emit(out, f"D/edge_{'shift' if shift else 'noshift'}/{h}x{w}/{tag}/{kind}", image(kind, h, w, rng), lst, entries, where,
                      undercut, edge=True, shift=shift)
    # partial water levels on noise: the tiles do not fill (no claim), except at 3 x 3, whose only interior pixel is the seed
    for shape in D_SHAPES:
        h, w = shape
        for lvl in (31, 100):
            rng = _rng(f"D/level{lvl}/{h}x{w}")
            for tag, lst, entries, where, _ in _lists(shape, rng)[:1 if shape != (3, 3) else 2]:      # (3 x 3: centre twice, thrice)
                _emit(out, f"D/level{lvl}/{h}x{w}/{tag}/noise", image("noise", h, w, rng), lst, entries, where,
                      True if shape == (3, 3) else None, max_level=lvl)
    _D = out
    return out


# ---- family L: long runs of one-lake tiles -------------------------------------------------------------------------------------------

OPEN = 9


def _expand(pattern):
    """'O*3 X W*2' -> 'OOOXWW'."""
    s = ""
    for tok in pattern.split():
        c, _, k = tok.partition("*")
        s += c * (int(k) if k else 1)
    return s


def _tile_box(shape, ty, tx):
    return ty * UT, tx * UT, min(ty * UT + UT, shape[0]), min(tx * UT + UT, shape[1])


def _cross(shape, ty, tx):
    """Row and column of an X tile's corridors: through its middle, interior to the plane even where the tile is thin."""
    y0, x0, y1, x1 = _tile_box(shape, ty, tx)
    return y0 + (y1 - y0 - 1) // 2, x0 + (x1 - x0 - 1) // 2


def l_plane(name, shape, rows, seeds):
    """rows: one pattern per tile row; seeds: (ty, tx, pos) in colour order, pos 'l', 'c' or 'r': where in an open tile the seed
    sits (an X tile: on the crossing of its corridors)."""
    h, w = shape
    rows = [_expand(r) for r in rows]
    ty, tx = (h + UT - 1) // UT, (w + UT - 1) // UT
    assert len(rows) == ty and all(len(r) == tx for r in rows), (name, ty, tx, [len(r) for r in rows])
    img = np.full(shape, OPEN, dtype=np.uint8)
    for y in range(ty):
        for x in range(tx):
            y0, x0, y1, x1 = _tile_box(shape, y, x)
            if rows[y][x] in "XW":
                img[y0:y1, x0:x1] = NEVER_FILL
            if rows[y][x] == "X":
                cy, cx = _cross(shape, y, x)
                img[cy, x0:x1] = OPEN
                img[y0:y1, cx] = OPEN
    pts = []
    for (y, x, pos) in seeds:
        y0, x0, y1, x1 = _tile_box(shape, y, x)
        assert rows[y][x] != "W", (name, y, x)
        if rows[y][x] == "X":
            pts.append(_cross(shape, y, x))
        else:
            pts.append((y0 + min(20, (y1 - y0 - 1) // 2), x0 + min({"l": 4, "c": 32, "r": 59}[pos], x1 - x0 - 2)))
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
    assert len(pts) <= 13 and (pts[:, 0] >= 1).all() and (pts[:, 0] <= h - 2).all() and (pts[:, 1] >= 1).all() and (pts[:, 1] <= w - 2).all(), name
    facts = {"family": "L", "edge": False, "shift": False, "max_level": 254, "pattern": rows}
    return (f"L/{h}x{w}/{name}", img, pts, facts)


_L = None


def l_cases():
    global _L
    if _L is not None:
        return _L
    out = []
    # one tile row of 70: a run from lane 0, one whose smallest colour sits in its first tile, and one from lane 62 that crosses
    # the wave boundary at tile 64, its smallest colour beyond it (tile 67); two solid tiles: three lakes
    out.append(l_plane("row70", (64, 4480), ["O*3 X O*27 W O*18 W O*10 X O*8"],
                       [(0, 67, "c"), (0, 4, "l"), (0, 5, "l"), (0, 62, "c"), (0, 64, "c"), (0, 40, "c"), (0, 1, "c"), (0, 55, "r")]))
    # one tile row of 130: heads at lanes 1 and 63; the run from tile 63 crosses two wave boundaries and has its smallest
    # colour in its last tile alone
    out.append(l_plane("row130", (64, 8320), ["X O*40 W O*20 X O*67"],
                       [(0, 129, "r"), (0, 128, "r"), (0, 100, "c"), (0, 63, "l"), (0, 20, "c"), (0, 45, "c"), (0, 70, "c"), (0, 1, "l")]))
    # 13 rows of 5: the wave boundary (tile 64) falls inside row 12; upper runs start left of, at and right of the run below
    out.append(l_plane("13x5", (832, 320),
                       ["O*5", "X O*3 X", "X O*4", "O*3 X O", "W*5", "O*2 X O*2", "O X O*3", "O*5", "X*2 O X*2", "O*5", "W*5", "O*5", "W X O*3"],
                       [(12, 4, "r"), (12, 2, "l"), (0, 0, "c"), (3, 4, "c"), (2, 2, "c"), (5, 0, "c"), (7, 3, "r"), (9, 1, "c"), (6, 4, "c"),
                        (11, 0, "l"), (1, 2, "c"), (8, 2, "c")]))
    # 3 rows of 44: wave boundaries at (1, 20) and (2, 40)
    out.append(l_plane("3x44", (192, 2816), ["X O*20 W O*22", "O*10 X O*33", "W*5 O*39"],
                       [(2, 43, "r"), (1, 30, "c"), (0, 1, "l"), (0, 30, "c"), (1, 0, "c"), (2, 10, "c"), (1, 15, "l"), (2, 38, "c"), (0, 43, "c"),
                        (1, 21, "r")]))
    # thin last tile row (2 rows: a corridor would open its only interior row) and column (3 columns)
    out.append(l_plane("thin", (194, 323), ["O*6", "O X O*2 W O", "O*3 X O*2", "O*2 W O*3"],
                       [(3, 5, "c"), (0, 0, "c"), (1, 5, "c"), (3, 0, "l"), (2, 3, "c"), (1, 1, "c"), (0, 5, "r"), (3, 3, "c")]))
    _L = out
    return out


def all_cases():
    return d_cases() + l_cases()


def named(prefix):
    got = [c for c in all_cases() if c[0].startswith(prefix)]
    assert len(got) == 1, (prefix, [c[0] for c in got])
    return got[0]
