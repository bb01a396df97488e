"""The inputs tests/test_lake_shapes_cpu.py proves things about and tests/test_gpu_lake_shapes.py runs, each with its reference
(tests/lake_shapes_ref.py) computed once per process and never changed."""
import functools
import os
import re

import numpy as np

import cases
import extreme_cases as xc
import lake_shapes_ref as sh
import lake_stats_ref as ls
import merge_tree_ref as mt
import merging_cases as mc
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THIN = [(8, 70001), (70001, 8)]      # the smallest planes of extreme_cases' tier A with a sum >= 2^64 (columns; rows)
THIN_MAX_LEVEL = 100
LINE = (3, (1 << 24) + 300)          # the closed-form plane: a coordinate past 2^24 (with u16 weights the stats call refuses it)


class Ref:
    """One call with everything the oracle says about it: planes, ps, tree (n + 1, 4), parent, death, ex, v, sums and (lazily) stats."""

    def __init__(self, img, seeds, weights=None, max_level=254, edge=False, seed_shift=False, keep_planes=True):
        self.img, self.seeds, self.weights = np.ascontiguousarray(img, dtype=np.uint8), np.asarray(seeds, dtype=np.int64).reshape(-1, 2), weights
        self.max_level, self.edge, self.seed_shift = max_level, edge, seed_shift
        planes, self.ps = mt.oracle_planes(self.img, self.seeds, max_level, edge, seed_shift)
        self.parent, self.death, area, leaves, _, self.ex = mt.tree_from_planes(planes, self.ps)
        self.tree = np.stack([self.parent, self.death, area, leaves], axis=1)
        self.v = ls.plane_weights(self.img, weights, edge)
        self.sums = sh.shapes_from_planes(planes, self.ps, self.v, self.death, self.ex)
        self.planes = planes if keep_planes else None

    @functools.cached_property
    def stats(self):
        """lake_stats_ref's records (only of a case that kept its planes)."""
        return ls.stats_from_planes(self.planes, self.ps, self.v, self.death, self.ex)


def u16_plane(shape, seed):
    """A u16 weight plane that holds 0 and 65535 several times."""
    rng = np.random.default_rng(4000 + seed)
    w = rng.integers(0, 65536, shape, dtype=np.uint16)
    flat = w.reshape(-1)
    where = rng.permutation(flat.size)
    flat[where[:max(flat.size // 50, 2)]] = 65535
    flat[where[-max(flat.size // 50, 2):]] = 0
    return w


def duplicate_seed_case():
    """Shuffled seeds with duplicates: a later seed on the same pixel overwrites, so some colours do not exist."""
    img = cases.field(40, 56, 21)
    seeds = np.asarray(ol.find_local_minima(img), dtype=np.int64)
    rng = np.random.default_rng(9)
    seeds = seeds[rng.permutation(len(seeds))]
    return img, np.concatenate([seeds[:7], seeds, seeds[3:5]])


def walled_case():
    """Walls of 255 cut the plane in rooms: record 0 is not empty; seeds touch at value 0, so some die at level 0."""
    img = cases.field(33, 47, 5)
    img[::8, :] = 255
    img[:, ::11] = 255
    img[3, 3] = img[3, 4] = 0
    return img, np.array([[3, 3], [3, 4], [12, 14], [20, 30], [29, 40], [12, 40]], dtype=np.int64)


def overflow_case():
    """The input of test_gpu_lake_stats.test_table_overflow_falls_back_to_memory: nothing floods, every seed of the checkerboard
    stays its own root, and each run of 1024 pixels holds 512 seed roots and root 0."""
    h, w = 32, 64
    img = np.full((h, w), 255, dtype=np.uint8)
    rr, cc = np.nonzero((np.add.outer(np.arange(h), np.arange(w)) & 1) == 0)
    return img, np.stack([rr, cc], axis=1), np.random.default_rng(3).integers(0, 65536, (h, w), dtype=np.uint16)


def three_seas_case():
    """5 x 70001, every weight 65535: three rooms of three rows at value 0 -- columns 1 .. 999 (colour 1), 1001 .. 43699 (colour 2)
    and 43701 .. 69999 (colour 3) -- behind doors of value 50 and 60, one seed in the middle of each.  2 dies at level 50 and 3 at
    level 60, both into 1.  The sum of v col^2 is 5.5e18 over the first two rooms and 1.70e19 over the third, each below 2^64 =
    1.84e19; record 1 holds their total, 2.25e19: its low word carries only when the two children are joined."""
    h, w = 5, 70001
    img = np.full((h, w), 255, dtype=np.uint8)
    img[1:-1, 1:-1] = 0
    img[1:-1, 1000] = img[1:-1, 43700] = 255
    img[2, 1000], img[2, 43700] = 50, 60
    return img, np.array([[2, 500], [2, 22000], [2, 57000]], dtype=np.int64), np.full((h, w), 65535, dtype=np.uint16)


def table_slots():
    """SHAPE_SLOTS as the kernels' header states it."""
    text = open(os.path.join(ROOT, "rustronomy-watershed_amd", "csrc", "ws_shape_part.hpp")).read()
    return int(re.search(r"SHAPE_SLOTS\s*=\s*(\d+)", text).group(1))


@functools.lru_cache(maxsize=None)
def small(name):
    """The small cases by name, with u16 weights unless the name says otherwise."""
    if name.startswith("field"):
        _, h, w, seed, edge, kind = name.split(":")
        shape = (int(h), int(w))
        img = cases.field(*shape, int(seed))
        wt = {"image": None, "u8": (u16_plane(shape, int(seed)) >> 8).astype(np.uint8), "u16": u16_plane(shape, int(seed))}[kind]
        return Ref(img, ol.find_local_minima(img), wt, edge=edge == "1")
    if name == "duplicates":
        img, seeds = duplicate_seed_case()
        return Ref(img, seeds, u16_plane(img.shape, 2))
    if name == "walls":
        img, seeds = walled_case()
        return Ref(img, seeds, u16_plane(img.shape, 3))
    if name == "three_seas":
        img, seeds, wt = three_seas_case()
        return Ref(img, seeds, wt, max_level=61)
    if name == "overflow":
        img, seeds, wt = overflow_case()
        return Ref(img, seeds, wt, max_level=2)
    for c in mc.constructed_cases():
        if c.name == name:
            return Ref(c.img, c.seeds, u16_plane(c.img.shape, 6), max_level=c.max_level, edge=c.edge, seed_shift=c.seed_shift)
    raise KeyError(name)


FIELDS = ["field:24:24:1:0:u16", "field:50:70:2:0:u8", "field:96:96:3:1:u16", "field:50:70:2:0:image"]
CONSTRUCTED = ["staircase", "plateau_w516", "plateau_w517", f"two_seas_max{mc.TWO_SEAS_V - 1}", f"two_seas_max{mc.TWO_SEAS_V}", "two_seas_max254"]
SMALL = FIELDS + ["duplicates", "walls", "overflow", "three_seas"] + CONSTRUCTED


@functools.lru_cache(maxsize=None)
def thin(shape):
    """A tier-A plane of extreme_cases with its u16 weights, flooded to THIN_MAX_LEVEL: by then one lake holds two thirds of the
    plane, and the oracle has 101 planes to hand over, not 255 (the planes themselves are dropped)."""
    img, seeds = xc.tier_a_input(shape)
    return Ref(img, seeds, xc.weights_u16(shape, 1), max_level=THIN_MAX_LEVEL, keep_planes=False)


def line_planes(shape=LINE):
    """The closed-form case as the arrival form takes it: one colour, stamp 0 on its seed pixel (0, 0) and level 1 elsewhere,
    every weight the largest of its type.  (keys, labels, u8 weights, u16 weights) as numpy planes."""
    keys = np.full(shape, 1 << 24, dtype=np.uint32)
    keys[0, 0] = 0
    return keys, np.ones(shape, dtype=np.uint32), np.full(shape, 255, dtype=np.uint8), np.full(shape, 65535, dtype=np.uint16)


def accepted(ph, pw, wmax):
    """check_lake_weights' bound as ws_lists.hip computes it: the stats call takes the plane."""
    pixels, longest = ph * pw, max(ph, pw)
    return not (longest and pixels > ((1 << 64) - 1) // wmax // longest)
