"""The cubes tests/test_lake_shapes_batch_cpu.py proves things about and tests/test_gpu_lake_shapes_batch.py runs through
ws_merge_tree_shapes_batch(_device), each with its per-slice reference (tests/lake_shapes_ref.py over the CPU oracle's planes, or a
closed form) computed once per process and never changed."""
import functools

import numpy as np

import lake_shapes_cases as lc
import lake_shapes_ref as sh
import lake_stats_batch_cases as bc
import lake_stats_ref as ls
import merge_tree_ref as mt
import oracle_lib as ol

STEP = bc.STEP      # pixels a workgroup of the own-shapes kernel takes per step (k_lake_own's grid)
HIGH_SHAPE = (2, 8, 70016)      # a plane of 4376 * 128 pixels with a side past 65 535: it stacks, and is not FLAT
HIGH_SEEDS = [(3, 100), (5, 60000)]
KINDS = ("image", "u8", "u16")


class Cube:
    """One call: the slices, their seed lists, the weight cube (None: the cube itself) and the options."""

    def __init__(self, imgs, lists, weights=None, max_level=254, edge=False, seed_shift=False):
        self.imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in imgs]
        self.lists = [np.asarray(l, dtype=np.int64).reshape(-1, 2) for l in lists]
        self.weights, self.max_level, self.edge, self.seed_shift = weights, max_level, edge, seed_shift

    @property
    def shape(self):
        return (len(self.imgs),) + self.imgs[0].shape

    @property
    def plane(self):
        """The padded plane of one slice: (rows, columns)."""
        e = 2 if self.edge else 0
        return self.imgs[0].shape[0] + e, self.imgs[0].shape[1] + e

    def stacks(self):
        """stackable()'s conditions on the shape (the seeds of these cubes are sorted and every cube has one)."""
        ph, pw = self.plane
        return len(self.imgs) > 1 and pw % 4 == 0 and (ph * pw) % 128 == 0

    def first(self):
        """First record of every slice, and the total: slice k's n_k + 1 records start at (seeds before it) + k."""
        at = [0]
        for l in self.lists:
            at.append(at[-1] + len(l) + 1)
        return at

    def slice_weights(self, k):
        return None if self.weights is None else self.weights[k]


class SliceRef:
    """What the oracle says about one slice: tree (n + 1, 4), stats records, sums (n + 1, 6), and the planes' pixel owners."""

    def __init__(self, cube, k):
        planes, ps = mt.oracle_planes(cube.imgs[k], cube.lists[k], cube.max_level, cube.edge, cube.seed_shift)
        parent, death, area, leaves, _, ex = mt.tree_from_planes(planes, ps)
        v = ls.plane_weights(cube.imgs[k], cube.slice_weights(k), cube.edge)
        self.tree = np.stack([parent, death, area, leaves], axis=1)
        self.death, self.ex, self.ps = death, ex, ps
        self.stats = ls.stats_from_planes(planes, ps, v, death, ex)
        self.sums = sh.shapes_from_planes(planes, ps, v, death, ex)
        stack = np.stack([np.asarray(p).astype(np.int64) for p in planes])
        arrival = np.argmax(stack != 0, axis=0)
        self.owner = np.take_along_axis(stack, arrival[None], axis=0)[0]      # a pixel's root at its arrival level, 0: never coloured


def _weights(shape, kind, seed):
    return dict(bc.weight_cubes(shape, seed))[kind]


def high_word_weights():
    """u16 weights of HIGH_SHAPE that differ by slice and by row: 65535 - 16 * slice - row."""
    s, h, w = HIGH_SHAPE
    wt = np.empty(HIGH_SHAPE, dtype=np.uint16)
    for k in range(s):
        for r in range(h):
            wt[k, r, :] = 65535 - 16 * k - r
    return wt


def rect_sums(row_weights, r0, r1, c0, c1):
    """The six sums over rows r0 .. r1 - 1 and columns c0 .. c1 - 1 of a plane whose row r weighs row_weights[r] everywhere,
    in closed form over the columns (as lake_shapes_ref.closed_form_line_plane)."""
    s1 = lambda n: n * (n - 1) // 2
    s2 = lambda n: (n - 1) * n * (2 * n - 1) // 6
    n, c1s, c2s = c1 - c0, s1(c1) - s1(c0), s2(c1) - s2(c0)
    out = [0] * 6
    for r in range(r0, r1):
        v = int(row_weights[r])
        out[0] += v * r * r * n
        out[1] += v * c2s
        out[2] += v * r * c1s
        out[3] += r * r * n
        out[4] += c2s
        out[5] += r * c1s
    return out


def high_word_expected(k):
    """Slice k of the high-word cube in closed form: the image is 0 everywhere, so the one seed floods the interior at level 0
    and never dies; the border is never coloured.  (tree rows, sums): record 0 the border, record 1 the interior."""
    _, h, w = HIGH_SHAPE
    rows = [65535 - 16 * k - r for r in range(h)]
    inner = rect_sums(rows, 1, h - 1, 1, w - 1)
    whole = rect_sums(rows, 0, h, 0, w)
    area = (h - 2) * (w - 2)
    tree = np.array([[0, mt.ALIVE, h * w - area, 0], [0, mt.ALIVE, area, 1]], dtype=np.int64)
    return tree, np.array([[a - b for a, b in zip(whole, inner)], inner], dtype=object)


@functools.lru_cache(maxsize=None)
def cube(name):
    """The cubes by name."""
    if name.startswith("shape:"):      # (a): lake_stats_batch_cases.SHAPES with each weight choice
        _, i, kind = name.split(":")
        shape, edge = bc.SHAPES[int(i)]
        imgs = bc.random_images(shape)
        return Cube(imgs, bc.seed_lists(imgs), _weights(shape, kind, 40), edge=edge)
    if name == "differ":      # (b): every slice with its own minima
        shape = (3, 40, 96)
        imgs = bc.random_images(shape, 4321)
        return Cube(imgs, [ol.find_local_minima(im) for im in imgs], _weights(shape, "u16", 41))
    if name == "high_word":      # (c)
        s, h, w = HIGH_SHAPE
        return Cube([np.zeros((h, w), dtype=np.uint8) for _ in range(s)], [[p] for p in HIGH_SEEDS], high_word_weights(), max_level=2)
    if name == "all_seeds":      # (d): every pixel a seed, in row-major order
        shape = (3, 8, 16)
        imgs = bc.random_images(shape, 4333)
        every = np.stack(np.divmod(np.arange(8 * 16), 16), axis=1)
        return Cube(imgs, [every] * 3, _weights(shape, "u16", 42))
    if name == "all255:small_checkerboard":      # (d): eight planes of 128 pixels in ONE step, 64 seeds each that never touch
        shape = (8, 8, 16)
        rr, cc = np.nonzero((np.add.outer(np.arange(8), np.arange(16)) & 1) == 0)
        seeds = np.stack([rr, cc], axis=1)
        return Cube([np.full(shape[1:], 255, dtype=np.uint8) for _ in range(8)], [seeds] * 8, _weights(shape, "u16", 78), max_level=3)
    if name.startswith("all255:"):
        shape, lists = bc.all_255_case(name.split(":")[1])
        return Cube([np.full(shape[1:], 255, dtype=np.uint8) for _ in range(shape[0])], lists, _weights(shape, "u16", 77), max_level=3)
    if name == "level0":      # (e)
        imgs, lists, _ = bc.level_zero_death_case()
        return Cube(imgs, lists, _weights((len(imgs),) + imgs[0].shape, "u16", 45))
    if name == "level0:edge":
        imgs, lists, _ = bc.level_zero_death_case()
        return Cube(imgs, lists, _weights((len(imgs),) + imgs[0].shape, "u8", 45), edge=True, seed_shift=True)
    if name == "empty0":
        imgs, lists, _ = bc.empty_record_zero_case()
        return Cube(imgs, lists, _weights((len(imgs),) + imgs[0].shape, "u16", 46))
    raise KeyError(name)


SHAPE_CASES = [f"shape:{i}:{kind}" for i in range(len(bc.SHAPES)) for kind in KINDS]
ORACLE_CASES = SHAPE_CASES + ["differ", "all_seeds", "all255:last_rows", "all255:checkerboard", "all255:small_checkerboard", "level0",
                             "level0:edge", "empty0"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The per-slice references (SliceRef) of an oracle case."""
    c = cube(name)
    return [SliceRef(c, k) for k in range(len(c.imgs))]


def expected_sums(name):
    """The call's shapes records as (total, 6) Python ints: every slice's, concatenated in the call's layout."""
    if name == "high_word":
        return np.concatenate([high_word_expected(k)[1] for k in range(HIGH_SHAPE[0])])
    return np.concatenate([r.sums for r in reference(name)])


def step_owners(name):
    """Per 1024-pixel step of the stacked plane: the set of (slice, owner) pairs -- the accumulator entries the step's
    workgroup meets (owner 0: the slice's own record 0)."""
    refs = reference(name)
    owner = np.concatenate([r.owner.ravel() for r in refs])
    which = np.repeat(np.arange(len(refs)), refs[0].owner.size)
    return [set(zip(which[i:i + STEP].tolist(), owner[i:i + STEP].tolist())) for i in range(0, owner.size, STEP)]
