"""Inputs that put the tiled transforms (csrc/ws_tiled.hip, csrc/ws_block_api.hip) where block code goes wrong: blocks of one
or two owned rows, seeds on seam and halo rows, ranks without seeds, floods that cross every seam dozens of times, plateaus whose
ring counts must agree across seams, and lakes whose pieces inside a block are joined only through other blocks.  Plain numpy,
seeded, no GPU.  tests/test_tiled_cases_cpu.py proves from the oracle that every family reaches its regime (and runs the
protocol on the numpy stand-in over gloo); tests/test_gpu_tiled_edges.py compares the HIP kernels with the oracle bit for bit.

Every generator returns a list of (name, image, seeds, world).  The name ends in the FORM the case is meant to take in
tiled_rank (csrc/ws_tiled.hip):

  /fast      w % 4 == 0 and the list strictly increasing in row-major order: seed tables, one table exchange for the labels
  /shuffled  the same field, the same seeds in another order (rows not sorted): explicit colours, the general form
  /wide      the same field with one more column of 255 (w % 4 == 1), the list as it was: the general form
  /dup       a seed twice (family c): not strictly increasing, the general form; the later entry's colour wins

Family g (edge correction) adds /noshift or /shift before the form: without the shift the list indexes the PADDED plane as it
stands (lib.rs:1675-1677), with it the list indexes the image and the engine moves it one pixel in; there the padded width
decides the form, so the fast cases have w % 4 == 2.
"""
import zlib

import numpy as np

FORMS = ("fast", "shuffled", "wide", "dup")


def tile_rows(h, rank, world):
    """(r0, r1, lo, hi) of ws_tile_rows / distributed.row_block: owned rows [r0, r1), local plane [lo, hi) with its halo rows."""
    assert 1 <= world <= h and 0 <= rank < world
    base, extra = divmod(h, world)
    r0 = rank * base + min(rank, extra)
    r1 = r0 + base + (1 if rank < extra else 0)
    return r0, r1, (r0 - 1 if rank > 0 else r0), (r1 + 1 if rank < world - 1 else r1)


def form_of(name):
    f = name.rsplit("/", 1)[1]
    assert f in FORMS, name
    return f


def edge_options(name):
    """(edge_correction, seed_shift) of a case, from its name."""
    return ("/noshift/" in name or "/shift/" in name), "/shift/" in name


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _sorted(seeds):
    s = np.asarray(seeds, dtype=np.int64).reshape(-1, 2)
    s = np.unique(s, axis=0)                  # lexicographic: row-major, strictly increasing
    return s


def is_strictly_increasing(seeds, w):
    s = np.asarray(seeds, dtype=np.int64).reshape(-1, 2)
    return bool((np.diff(s[:, 0] * w + s[:, 1]) > 0).all())


def _wide(img):
    out = np.full((img.shape[0], img.shape[1] + 1), 255, dtype=np.uint8)
    out[:, :-1] = img
    return out


def with_twin(name, img, seeds, world, twin=None):
    """The fast case and its general-form twin.  twin: "shuffled" (needs a list whose rows can be put out of order), "wide", or
    None: shuffled where the list allows it, wide otherwise."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    s = _sorted(seeds)
    assert img.shape[1] % 4 == 0 or edge_options(name + "/fast")[0], name
    out = [(name + "/fast", img, s, world)]
    can_shuffle = len(np.unique(s[:, 0])) >= 2
    if twin is None:
        twin = "shuffled" if can_shuffle else "wide"
    if twin == "shuffled":
        assert can_shuffle, name
        rng = _rng(name)
        p = s[rng.permutation(len(s))]
        if (np.diff(p[:, 0]) >= 0).all():     # a draw that left the rows in order: the reverse never does
            p = s[::-1].copy()
        assert (np.diff(p[:, 0]) < 0).any()
        out.append((name + "/shuffled", img, p, world))
    else:
        assert twin == "wide" and not edge_options(name + "/wide")[0]
        out.append((name + "/wide", _wide(img), s.copy(), world))
    return out


def _noise(rng, h, w):
    return rng.integers(0, 201, (h, w), dtype=np.uint8)


def _random_seeds(rng, h, w, n):
    n = max(1, min(n, h * w))
    flat = np.sort(rng.choice(h * w, size=n, replace=False))
    s = np.stack([flat // w, flat % w], axis=1).astype(np.int64)
    if h >= 2 and len(np.unique(s[:, 0])) < 2:      # (a shuffled twin needs two rows to put out of order)
        s = np.concatenate([s, [[h - 1 - int(s[0, 0] == h - 1), w // 2]]])
    return s


# ---- a: blocks of ONE owned row -------------------------------------------------------------------------------------------------

def one_row_blocks():
    out = []
    for world in (2, 3, 4, 8):
        for w in (4, 32, 260):
            name = f"a/{world}x{w}/world{world}"
            rng = _rng(name)
            h = world
            seeds = _random_seeds(rng, h, w, max(2, h * w // 6))
            out += with_twin(name, _noise(rng, h, w), seeds, world, twin="shuffled" if (world + w // 4) % 2 else "wide")
    return out


# ---- b: uneven thin blocks: some ranks own one row, others two ----------------------------------------------------------------

def thin_blocks():
    out = []
    widths = (32, 4, 260)
    for world in (2, 3, 4, 8):
        for k, h in enumerate((world + 1, 2 * world - 1, 2 * world)):
            w = widths[(k + world) % 3]
            name = f"b/{h}x{w}/world{world}"
            rng = _rng(name)
            out += with_twin(name, _noise(rng, h, w), _random_seeds(rng, h, w, max(3, h * w // 6)), world,
                             twin="wide" if (world + k) % 2 else "shuffled")
    return out


# ---- c: seeds on seam and halo rows ---------------------------------------------------------------------------------------------

SEAM_SHAPE = (24, 64)


def seam_rows(h, world):
    """Every rank's first and last owned row: with the neighbours' halo rows, the same set."""
    rows = set()
    for r in range(world):
        r0, r1, _, _ = tile_rows(h, r, world)
        rows |= {r0, r1 - 1}
    return sorted(rows)


def seam_seeds():
    h, w = SEAM_SHAPE
    cols = (0, 1, w - 2, w - 1)
    out = []
    for world in (3, 4):
        img = _noise(_rng(f"c/world{world}"), h, w)
        rows = seam_rows(h, world)
        base = [(r, c) for r in rows for c in cols]
        out += with_twin(f"c/seams/world{world}", img, base, world)
        # one middle rank whose local plane, halo rows included, holds no seed: the seam rows outside it, and the two rows next to it
        _, _, lo, hi = tile_rows(h, 1, world)
        keep = [r for r in rows + [lo - 1, hi] if not lo <= r < hi and 0 <= r < h]
        out += with_twin(f"c/empty_rank1/world{world}", img, [(r, c) for r in keep for c in cols], world)
        # every seed in the last rank's owned rows
        r0, r1, _, _ = tile_rows(h, world - 1, world)
        out += with_twin(f"c/last_rank_only/world{world}", img, [(r, c) for r in (r0, r1 - 1) for c in cols], world)
        # adjacent seeds astride every seam, away from the plane's edge too
        astride = [(r, c) for k in range(1, world) for r in (tile_rows(h, k, world)[0] - 1, tile_rows(h, k, world)[0]) for c in (30, 31)]
        out += with_twin(f"c/astride/world{world}", img, base + astride, world)
        # a seam seed twice: the later entry's colour wins (lib.rs:1675-1677)
        s = _sorted(base)
        dup = np.concatenate([s, s[len(s) // 2 + 1][None, :]])
        out.append((f"c/seams/world{world}/dup", img, dup, world))
    return out


# ---- d: a zigzag corridor: the flood crosses every seam once per corridor, in both directions ---------------------------------

def zigzag(h=130, w=92):
    cor = np.full((h, w), 255, np.uint8)
    for c in range(1, w - 1, 2):
        cor[1:h - 1, c] = 4
        cor[h - 2 if (c // 2) % 2 == 0 else 1, c + 1] = 4
    return cor


def zigzag_corridor():
    out = []
    for world in (2, 4):
        out += with_twin(f"d/zigzag/world{world}", zigzag(), [(1, 1)], world, twin="wide")
    return out


# ---- e: a plateau: rings in the dozens, the stamps' ring counts have to agree across seams ------------------------------------

def plateau():
    out = []
    img = np.full((33, 64), 9, dtype=np.uint8)
    for world in (3, 4):
        out += with_twin(f"e/centre/world{world}", img, [(16, 31)], world, twin="wide")
        out += with_twin(f"e/corners/world{world}", img, [(1, 1), (31, 62)], world, twin="shuffled")
    return out


# ---- f: linked lakes -------------------------------------------------------------------------------------------------------------

LINKED_SHAPES = ((12, 32, 4), (24, 64, 3), (40, 36, 4), (8, 32, 8))
LINKED_LEVELS = (254, 60)


def linked_field(h, w):
    """Walls of 255 and two vertical serpentines, one in the left half of the columns and one in the right: corridors on every
    second column from row 1 to row h - 2, neighbours joined alternately at the bottom and at the top.  Returns (image, corridor
    columns of the left lake, of the right lake)."""
    img = np.full((h, w), 255, dtype=np.uint8)
    val = lambda r, c: (7 * r + 3 * c) % 100 + 1
    halves = (list(range(1, w // 2 - 1, 2)), list(range(w // 2 + 1, w - 1, 2)))
    for cols in halves:
        for k, c in enumerate(cols):
            for r in range(1, h - 1):
                img[r, c] = val(r, c)
            if k + 1 < len(cols):
                r = h - 2 if k % 2 == 0 else 1
                img[r, c + 1] = val(r, c + 1)
    return img, halves[0], halves[1]


def linked_seeds(h, w, world, left, right):
    """Left lake: no seed in block 0, the first in a middle row of block 1 (an interior row of the block where it has three rows
    or more), one more in every block further down, each on another corridor.  Right lake: the last block only."""
    seeds = []
    for k in range(1, world):
        r0, r1, _, _ = tile_rows(h, k, world)
        r = min(max(r0 + (r1 - r0) // 2, 1), h - 2)
        seeds.append((r, left[(5 * (k - 1)) % len(left)]))
    r0, r1, _, _ = tile_rows(h, world - 1, world)
    r = min(max(r0, 1), h - 2)
    seeds += [(r, right[0]), (min(r + 1, h - 2), right[len(right) // 2]), (r, right[-1])]
    return _sorted(seeds)


def linked_lakes():
    out = []
    for h, w, world in LINKED_SHAPES:
        img, left, right = linked_field(h, w)
        out += with_twin(f"f/{h}x{w}/world{world}", img, linked_seeds(h, w, world, left, right), world,
                         twin="shuffled" if w % 8 == 0 else "wide")
    return out


# ---- g: families a and f with edge correction -------------------------------------------------------------------------------------

def edge_correction():
    """The padded plane is (h + 2) x (w + 2): 2 x 32 over 4 ranks is 4 rows, so rank 0 owns only the virtual ring row.  w % 4 == 2
    pads to a fast width; w % 4 == 0 is the general form by its width, whatever the list."""
    out = []

    def both(tag, img, seeds_img, world):
        h, w = img.shape
        s = _sorted(seeds_img)
        for shift in (False, True):
            # without the shift the caller's list names pixels of the padded plane: the same pixels as with it, one further in
            lst = s if shift else s + 1
            name = f"g/{tag}/{h}x{w}/world{world}/{'shift' if shift else 'noshift'}"
            if (w + 2) % 4 == 0:
                out.extend(with_twin(name, img, lst, world, twin="shuffled"))
            else:
                rng = _rng(name)
                p = lst[rng.permutation(len(lst))]
                out.append((name + "/wide", img, lst, world))
                out.append((name + "/shuffled", img, p, world))

    for h, w, world in ((2, 32, 4), (2, 30, 4), (6, 30, 8), (3, 258, 4)):
        rng = _rng(f"g/a/{h}x{w}")
        seeds = _random_seeds(rng, h, w, max(3, h * w // 6))
        both("a", _noise(rng, h, w), seeds, world)
    for h, w, world in ((12, 30, 4), (12, 32, 4)):
        img, left, right = linked_field(h, w)
        both("f", img, linked_seeds(h, w, world, left, right), world)
    return out


def padded_equivalent(img, seeds, seed_shift):
    """The plain (no edge correction) call that an edge-corrected one equals: the image with a ring of zeros, the list moved with
    the shift or as it stands without (the construction of test_tiled_edge_correction_and_seed_shift)."""
    pad = np.zeros((img.shape[0] + 2, img.shape[1] + 2), np.uint8)
    pad[1:-1, 1:-1] = img
    s = np.asarray(seeds, dtype=np.int64).reshape(-1, 2)
    return pad, (s + 1 if seed_shift else s)


FAMILIES = {"a": one_row_blocks, "b": thin_blocks, "c": seam_seeds, "d": zigzag_corridor, "e": plateau, "f": linked_lakes,
            "g": edge_correction}


def family(letter):
    return FAMILIES[letter]()


def all_cases(letters="abcdefg"):
    return [c for l in letters for c in family(l)]
