"""The inputs of tests/test_gpu_lake_stats_batch.py, built with numpy alone so that tests/test_lake_stats_batch_cpu.py can prove,
without a GPU, that they reach the regimes the GPU tests name."""
import numpy as np

import cases
import lake_stats_ref as ls
import oracle_lib as ol

# as SHAPES of tests/test_gpu_merge_tree_batch.py: the stack's plane (padded with edge correction) is 128 x 96, or 40 x 96 = 3840
# pixels, whose 1024-pixel steps of the own-statistics pass straddle slices; no stack: w' % 4 != 0
SHAPES = [((6, 128, 96), False), ((6, 126, 94), True), ((5, 40, 96), False), ((5, 130, 98), False), ((5, 130, 98), True)]
STEP = 1024      # pixels a workgroup of the own-statistics kernel takes per step


def random_images(shape, seed=4000):
    s, h, w = shape
    return [cases.field(h, w, seed + 7 * k) for k in range(s)]


def seed_lists(imgs):
    """The slices' own minima, except: slice 1 has no seed, slice 2 a single one."""
    lists = [np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2) for im in imgs]
    lists[1] = lists[1][:0]
    lists[2] = lists[2][:1]
    return lists


def weight_cubes(shape, seed):
    """The three weight choices for a cube: none (the cube itself weighs: many ties), a u8 cube, and a u16 cube whose every
    slice is drawn from a generator seed of its own and uses 0 and 65535 several times each -- no plane a function of the image
    or of another slice's plane."""
    s, h, w = shape
    u8 = np.random.default_rng(9000 + seed).integers(0, 256, shape, dtype=np.uint8)
    u16 = np.empty(shape, dtype=np.uint16)
    for k in range(s):
        rng = np.random.default_rng(1000 * seed + 31 * k + 5)
        plane = rng.integers(0, 65536, h * w, dtype=np.uint16)
        where = rng.permutation(h * w)
        plane[where[:max(h * w // 50, 2)]] = 65535
        plane[where[-max(h * w // 50, 2):]] = 0
        u16[k] = plane.reshape(h, w)
    return [("image", None), ("u8", u8), ("u16", u16)]


def all_255_case(case):
    """(shape, seed lists) for an image of 255s, where nothing floods.  last_rows: (5, 40, 96), two or three seeds a slice, those
    of slice 1 and two of slice 2 in the last rows -- the 1024-pixel step that holds them also holds the first pixels of the next slice
    (a slice is 3840 pixels: slices 0, 1 and 2 end inside a step, slice 3 ends on one).
    checkerboard: (2, 32, 64) with the 1024 seeds (r + c) even in every slice -- a workgroup meets 512 seed roots and one record
    0 (the slices are 2048 pixels: a step never straddles here), one key more than the table's 512 slots."""
    if case == "checkerboard":
        rr, cc = np.nonzero((np.add.outer(np.arange(32), np.arange(64)) & 1) == 0)
        seeds = np.stack([rr, cc], axis=1).astype(np.int64)
        return (2, 32, 64), [seeds, seeds.copy()]
    lists = [np.array([[3, 5], [20, 77]], np.int64),
             np.array([[38, 2], [38, 90], [39, 95]], np.int64),
             np.array([[1, 1], [38, 40], [39, 30]], np.int64),
             np.array([[17, 50], [39, 0]], np.int64),
             np.array([[0, 0], [39, 95]], np.int64)]
    return (5, 40, 96), lists


def all_255_expected(weights, seeds):
    """The records of one slice of an all-255 image in closed form: every seed's record is its own pixel, record 0 every other
    pixel of the slice."""
    v = np.asarray(weights).astype(np.int64)
    want = ls.empty_records(len(seeds) + 1)
    plane = np.zeros(v.shape, dtype=np.int64)
    for k, (r, c) in enumerate(seeds):
        want[k + 1] = ls.pixel_record(v, int(r), int(c))
        plane[r, c] = 1
    want[0] = ls.records_by_label(plane, v, 2)[0]
    return want


def level_zero_death_case():
    """(images, seed lists, [(slice, colour)]): (4, 40, 96) random slices with their own minima; in slices 1 and 3 two more seeds
    on adjacent interior pixels of value 0, appended in row-major order after a prefix of the minima -- they touch before anything
    floods, so the later of the two dies at level 0 into the earlier."""
    shape = (4, 40, 96)
    imgs = random_images(shape, 4250)
    lists = []
    dying = []
    for k, im in enumerate(imgs):
        if k in (1, 3):
            im[20, 30 + k] = im[20, 31 + k] = 0
        mins = np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2)
        if k in (1, 3):
            a, b = (20, 30 + k), (20, 31 + k)
            keep = [tuple(p) for p in mins if tuple(p) not in (a, b)]
            both = sorted(keep + [a, b])
            mins = np.array(both, dtype=np.int64)
            dying.append((k, both.index(b) + 1))
        lists.append(mins)
    return imgs, lists, dying


def empty_record_zero_case():
    """(images, seed lists, slice): (3, 8, 16) -- a plane of 128 pixels, the smallest that stacks.  Slice 1 is 0 everywhere with a
    seed on every border pixel: the interior floods at level 0 and no pixel of the slice stays uncoloured, so its record 0 is the
    identity, between two random slices whose border is never coloured."""
    shape = (3, 8, 16)
    imgs = random_images(shape, 4270)
    imgs[1] = np.zeros((8, 16), dtype=np.uint8)
    lists = [np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2) for im in imgs]
    rr, cc = np.nonzero(np.pad(np.zeros((6, 14), dtype=bool), 1, constant_values=True))
    lists[1] = np.stack([rr, cc], axis=1).astype(np.int64)
    return imgs, lists, 1
