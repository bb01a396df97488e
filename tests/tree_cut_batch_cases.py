"""The inputs and the expected outputs of tests/test_gpu_tree_cut_batch.py, built with numpy and the CPU oracle alone so that
tests/test_tree_cut_batch_cpu.py can prove, without a GPU, that they reach the regimes the GPU tests name.  Expected values are
tests/tree_cut_catalogue_ref.py per slice, concatenated; a slice without seeds has its closed form (nothing shown, every pixel
hidden).  Every cube is built once per process and never changed afterwards."""
import numpy as np

import lake_stats_batch_cases as bc
import lake_stats_ref as ls
import merging_cases as mc
import oracle_lib as ol
import tree_cut_catalogue_ref as cc
import tree_cut_ref as tc
import tree_cut_stats_ref as ts

Cut = ts.Cut
RUN = 1024      # pixels of one step of a workgroup
ALIVE = tc.ALIVE


class Seedless:
    """A slice without seeds as the cut sees it: one record nobody reads, no colour, every pixel hidden."""

    def __init__(self, name, img, weights, edge):
        self.name, self.img, self.weights, self.edge, self.n_seeds = name, np.ascontiguousarray(img, dtype=np.uint8), weights, bool(edge), 0
        e = 2 if edge else 0
        self.shape = (img.shape[0] + e, img.shape[1] + e)
        self.seg = np.zeros(self.shape, dtype=np.uint32)
        self.tree = np.array([[0, ALIVE, self.shape[0] * self.shape[1], 0]], dtype=np.uint32)
        self.stats = ls.empty_records(1)
        self.seeds = np.zeros((0, 2), dtype=np.int64)

    def keys32(self):
        return np.full(self.shape, 0xFF000000, dtype=np.uint32)

    def cut(self, cut):
        return self.seg


def expected_slice(f, cuts):
    """(planes, lakes, region records, offsets, hidden, hidden records) of one slice alone."""
    if f.n_seeds == 0:
        whole = cc.whole_plane(f)
        hid = ls.empty_records(len(cuts))
        hid[:] = whole
        n = f.shape[0] * f.shape[1]
        return ([f.seg] * len(cuts), np.zeros((0, 2), np.uint64), ls.empty_records(0), np.zeros(len(cuts) + 1, np.uint64),
                np.full(len(cuts), n, np.uint64), hid)
    return ([f.cut(c) for c in cuts],) + tuple(cc.expected(f, cuts))


class Cube:
    """Slices of one shape with their seed lists and an optional weight cube, each flooded by the oracle."""

    def __init__(self, name, imgs, lists, weights=None, edge=False, cuts=()):
        self.name, self.imgs, self.lists, self.weights, self.edge = name, imgs, lists, weights, bool(edge)
        self.slices = []
        for k, (im, seeds) in enumerate(zip(imgs, lists)):
            wt = None if weights is None else weights[k]
            if len(seeds) == 0:
                self.slices.append(Seedless(f"{name}[{k}]", im, wt, edge))
            else:
                self.slices.append(ts.Field(f"{name}[{k}]", tc.Field(f"{name}[{k}]", im, seeds, edge=edge), wt))
        self.cuts = list(cuts)
        self._expected = {}

    @property
    def n_slices(self):
        return len(self.slices)

    @property
    def plane_shape(self):
        return self.slices[0].shape

    def seed_offsets(self):
        return [0] + [int(x) for x in np.cumsum([f.n_seeds for f in self.slices])]

    def first_records(self):
        offs = self.seed_offsets()
        return [offs[k] + k for k in range(len(offs))]

    def tree(self):
        return np.ascontiguousarray(np.concatenate([f.tree for f in self.slices]).astype(np.uint32))

    def stats_raw(self):
        return np.ascontiguousarray(np.concatenate([np.asarray(f.stats) for f in self.slices])).view(np.int64).reshape(-1, 9)

    def keys(self):
        return np.ascontiguousarray(np.stack([f.keys32() for f in self.slices]))

    def seg(self):
        return np.ascontiguousarray(np.stack([f.seg for f in self.slices]))

    def plane_weights(self):
        """The weights over the planes as (A) takes them: the planes' shape, the ring 0 under edge correction; u16 for a u16 cube."""
        dt = np.uint16 if self.weights is not None and self.weights.dtype == np.uint16 else np.uint8
        return np.ascontiguousarray(np.stack([cc.weights_of(f) for f in self.slices]).astype(dt))

    def expected(self, cuts=None):
        """Per slice, in order: (planes, lakes, region, offsets, hidden, hidden records), each slice's own, offsets from 0."""
        cuts = self.cuts if cuts is None else cuts
        key = tuple(c.key() for c in cuts)
        if key not in self._expected:
            self._expected[key] = [expected_slice(f, cuts) for f in self.slices]
        return self._expected[key]

    def expected_flat(self, cuts=None):
        """The caller's layout: (lakes, region, offsets (S * K + 1), hidden (S * K), hidden records (S * K))."""
        per = self.expected(cuts)
        lakes = np.concatenate([p[1] for p in per]).reshape(-1, 2)
        region = np.concatenate([p[2] for p in per])
        offsets, at = [], 0
        for p in per:
            offsets += [at + int(o) for o in p[3][:-1]]
            at += int(p[3][-1])
        offsets.append(at)
        return (lakes, region, np.array(offsets, np.uint64), np.concatenate([p[4] for p in per]).astype(np.uint64), np.concatenate([p[5] for p in per]))


def exact_area(f):
    """An area some dead node of the flood has: a min_area threshold that is met exactly."""
    dead = f.area[1:][f.death[1:] != ALIVE]
    return int(np.sort(dead)[len(dead) // 2]) if len(dead) else 0


def generic_cuts(f):
    """Cuts that move only the table (thresholds, merge_level 0), only the walk (no threshold, levels) and both; one threshold is
    met exactly by a node of slice f; two need the catalogue."""
    a = exact_area(f)
    return [Cut(), Cut(min_area=a), Cut(min_area=a + 1), Cut(show_level=254, merge_level=90), Cut(show_level=110, merge_level=0),
            Cut(min_area=a, show_level=200, merge_level=60), Cut(min_leaves=2, merge_level=30), Cut(min_depth=12, min_w_max=1),
            Cut(min_sum_w=int(np.median(f.stats["sum_w"][1:][f.death[1:] != ALIVE])) or 1, merge_level=20)]


def _u16_one_slice(shape, seed, big):
    """A u16 weight cube whose slice `big` uses the whole range and whose other slices stay below 256."""
    wt = [w for n, w in bc.weight_cubes(shape, seed) if n == "u16"][0].copy()
    for k in range(shape[0]):
        if k != big:
            wt[k] &= 0xFF
    return wt


def record_ok(tree, i, lo=0):
    """k_cut_check's rule for record i of `tree` read as ONE tree whose record 0 is at lo."""
    parent, death, c = int(tree[i, 0]), int(tree[i, 1]), i - lo
    if death == ALIVE:
        return parent == 0
    return death <= 254 and 0 < parent < c and int(tree[lo + parent, 1]) > death


def slice_verdict(cube, tree):
    """The rule within every slice (the record of a slice without seeds is not read): what the cube call says of the records."""
    first = cube.first_records()
    return all(record_ok(tree, i, first[k]) for k, f in enumerate(cube.slices) if f.n_seeds for i in range(first[k], first[k + 1]))


def foreign_parent(cube):
    """(index i in the whole array, parent p): a dead record of a late slice given a parent ABOVE its own colour that the whole
    array, read as one tree, accepts: p < i and record p of the whole array dies later."""
    tree, first = cube.tree(), cube.first_records()
    for k in range(2, cube.n_slices):
        n_k = cube.slices[k].n_seeds
        for c in range(1, n_k):
            i = first[k] + c
            if tree[i, 1] == ALIVE:
                continue
            for p in range(c + 1, n_k + 1):
                if p < i and int(tree[p, 1]) > int(tree[i, 1]):
                    return i, p
    raise AssertionError("no such record")


_CUBES = {}


def _minima(img):
    return np.asarray(ol.find_local_minima(img), dtype=np.int64).reshape(-1, 2)


def _random(name, shape, edge, weights, seed):
    imgs = bc.random_images(shape, seed)
    lists = bc.seed_lists(imgs)
    wt = None
    if weights == "u8":
        wt = [w for n, w in bc.weight_cubes(shape, seed) if n == "u8"][0]
    elif weights == "u16":
        wt = _u16_one_slice(shape, seed, 3)
    cube = Cube(name, imgs, lists, wt, edge)
    # (the thresholds come from the first slice in which a lake dies: a tiny slice may have none)
    dying = [f for f in cube.slices if f.n_seeds and exact_area(f)]
    cube.cuts = generic_cuts(dying[0] if dying else cube.slices[0])
    return cube


def _tiny():
    """(5, 5, 7): 35-pixel planes, whose quads straddle slices and whose every slice but the first is off 16-byte alignment.  The
    minima of so small a plane are one or none, so the seeds are planted: five to seven a slice, two of them
    on its first and last pixel (so that a quad across two slices shows pixels of both), slice 1 without."""
    imgs = bc.random_images((5, 5, 7), 4340)
    spots = [(1, 1), (1, 4), (2, 6), (3, 2), (3, 5)]
    corners = [(0, 0), (4, 6)]      # the first and the last pixel of a slice: border pixels are coloured only where a seed sits
    lists = [np.array(sorted(spots[k % 2: 3 + k % 3 + k % 2] + corners), dtype=np.int64).reshape(-1, 2) for k in range(5)]
    lists[1] = lists[1][:0]
    wt = [w for n, w in bc.weight_cubes((5, 5, 7), 4340) if n == "u8"][0]
    cube = Cube("5x5x7", imgs, lists, wt, False)
    dying = [f for f in cube.slices if f.n_seeds and exact_area(f)]
    cube.cuts = generic_cuts(dying[0])
    return cube


def _checkerboard():
    """(2, 32, 64) noise with a seed on every other pixel: 1024 regions a slice, more than half a table in a run."""
    import seed_cases as sc
    r, c = np.indices((32, 64))
    seeds = np.stack(np.nonzero((r + c) % 2 == 0), axis=1).astype(np.int64)
    imgs = [sc.image("noise", 32, 64, 81), sc.image("noise", 32, 64, 82)]
    cube = Cube("checkerboard", imgs, [seeds, seeds.copy()], None, False)
    cube.cuts = [Cut(show_level=254, merge_level=0), Cut(min_area=3), Cut(show_level=120, merge_level=40)]
    return cube


def _chain():
    """The 254-deep parent chain of merging_cases.staircase as slice 1 of a two-slice cube, next to a random slice of its shape."""
    st = mc.staircase()
    other = bc.random_images((1,) + st.img.shape, 4400)[0]
    lists = [_minima(other), np.asarray(st.seeds, dtype=np.int64)]
    cube = Cube("chain", [other, st.img], lists, None, False)
    cube.cuts = [Cut(), Cut(show_level=254, merge_level=254), Cut(min_area=700, merge_level=100), Cut(min_leaves=200)]
    return cube


def _thirty_two():
    cube = _random("thirty_two", (5, 40, 96), False, "u8", 4100)
    cube.cuts = list(cc.THIRTY_TWO)
    return cube


_BUILDERS = {
    "9x8x16": lambda: _random("9x8x16", (9, 8, 16), False, "u8", 4300),
    "5x40x96": lambda: _random("5x40x96", (5, 40, 96), False, "u16", 4310),
    "6x126x94_edge": lambda: _random("6x126x94_edge", (6, 126, 94), True, None, 4320),
    "5x130x98": lambda: _random("5x130x98", (5, 130, 98), False, "u16", 4330),
    "5x5x7": _tiny,
    "checkerboard": _checkerboard,
    "chain": _chain,
    "thirty_two": _thirty_two,
}
STACKING = ["9x8x16", "5x40x96", "6x126x94_edge", "checkerboard"]      # planes that (B) floods as stacks
LOOPING = ["5x130x98"]                                                  # ... and one it loops over
DEVICE_ONLY = ["5x5x7", "chain", "thirty_two"]                          # (A) alone


def cube(name):
    if name not in _CUBES:
        _CUBES[name] = _BUILDERS[name]()
    return _CUBES[name]


TILED_SLICES = 65537


def tiled():
    """(the three distinct slices as a Cube, the index of the distinct slice every one of the 65 537 slices of 8 x 16 is, two cuts)."""
    if "tiled" not in _CUBES:
        imgs = bc.random_images((3, 8, 16), 4350)
        _CUBES["tiled"] = Cube("tiled", imgs, [_minima(im) for im in imgs], None, False)
    base = _CUBES["tiled"]
    which = (np.arange(TILED_SLICES) * 7 + np.arange(TILED_SLICES) // 3) % 3
    return base, which, [Cut(), Cut(min_area=exact_area(base.slices[0]), merge_level=40)]
