"""The merge tree of the merging transform derived with numpy from the CPU oracle's per-level planes, following the definition
of ws_merge_tree (include/ws_hip.h) literally: what tests/test_gpu_merge_tree.py compares the engine's records against."""
import numpy as np

import oracle_lib as ol

ALIVE = 0xFFFFFFFF


def plane_seeds(seeds, edge=False, seed_shift=False):
    """The seed pairs in the coordinates of the (padded) plane: moved by (+1, +1) only with edge correction AND seed_shift."""
    s = np.asarray(seeds, dtype=np.int64).reshape(-1, 2)
    return s + 1 if (edge and seed_shift) else s


def oracle_planes(img, seeds, max_level=254, edge=False, seed_shift=False):
    """P_0 .. P_max: the canonical merging planes (smallest seed colour of the lake), as tests/test_gpu_history.py takes them."""
    ps = plane_seeds(seeds, edge, seed_shift)
    snaps = []
    ol.merge(img, ps, max_level=max_level, edge=edge, hook=lambda l, m, i, c: snaps.append(ol.canonicalise(c, ps)[0]))
    assert len(snaps) == max_level + 1
    return snaps, ps


def existing(ps, shape):
    """exists[c]: colour c's seed pixel carries c right after seeding (a later duplicate overwrites, lib.rs:1670-1677)."""
    paint = np.zeros(shape, dtype=np.int64)
    for i, (r, c) in enumerate(ps):
        paint[r, c] = i + 1
    ex = np.zeros(len(ps) + 1, dtype=bool)
    for i, (r, c) in enumerate(ps):
        ex[i + 1] = paint[r, c] == i + 1
    return ex


def tree_from_planes(planes, ps):
    """(parent, death_level, area, n_leaves), uint32 arrays of n_seeds + 1, and seed_values[L, c] = P_L at c's seed pixel."""
    S = len(ps)
    shape = planes[0].shape
    ex = existing(ps, shape)
    parent = np.zeros(S + 1, dtype=np.uint32)
    death = np.full(S + 1, ALIVE, dtype=np.uint32)
    area = np.zeros(S + 1, dtype=np.uint32)
    leaves = np.zeros(S + 1, dtype=np.uint32)
    area[0] = int((planes[-1] == 0).sum())
    vals = np.zeros((len(planes), S + 1), dtype=np.int64)
    if S:
        for L, P in enumerate(planes):
            vals[L, 1:] = P[ps[:, 0], ps[:, 1]]
    px = {}      # level -> pixels per colour of P_level; seed pixels (of existing colours) per colour

    def counts(L):
        if L not in px:
            px[L] = (np.bincount(planes[L].ravel().astype(np.int64), minlength=S + 1),
                     np.bincount(vals[L, 1:][ex[1:]], minlength=S + 1))
        return px[L]

    for c in range(1, S + 1):
        if not ex[c]:
            continue
        gone = np.flatnonzero(vals[:, c] != c)
        if gone.size:
            L = int(gone[0])
            death[c] = L
            parent[c] = vals[L, c]
            before = L - 1
        else:
            before = len(planes) - 1
        if before < 0:
            area[c] = 1
            leaves[c] = 1
        else:
            area[c] = counts(before)[0][c]
            leaves[c] = counts(before)[1][c]
    return parent, death, area, leaves, vals, ex


def expected_tree(img, seeds, max_level=254, edge=False, seed_shift=False):
    planes, ps = oracle_planes(img, seeds, max_level, edge, seed_shift)
    return tree_from_planes(planes, ps)


def roots_at(parent, death, level):
    """colour -> the end of the walk along `parent` while death_level <= level.  The cap of 258 steps is enough for every valid
    tree: death levels strictly increase along `parent` and there are at most 255 levels, so no chain holds more than 255
    hooks -- the staircase of tests/merging_cases.py, 254 deep, comes within one of that (tests/test_merging_cases_cpu.py)."""
    root = np.arange(parent.size, dtype=np.int64)
    for _ in range(258):
        dead = death[root] <= level
        if not dead.any():
            return root
        root[dead] = parent[root[dead]]
    raise AssertionError("the parent walk does not end: a cycle, or a parent that does not die later")


def check_invariants(parent, death, area, leaves, vals=None, ex=None):
    """The three invariants of the tree: 0 < parent < c; the parent dies strictly later or never; the walk gives P_L at the seed
    pixel (where the seed pixels' values per level are at hand)."""
    parent = np.asarray(parent).astype(np.int64)
    death = np.asarray(death).astype(np.int64)
    c = np.arange(parent.size)
    dead = death != ALIVE
    assert not dead[0] and parent[0] == 0 and leaves[0] == 0
    assert (parent[dead] > 0).all() and (parent[dead] < c[dead]).all()
    assert (parent[~dead] == 0).all()
    assert (death[parent[dead]] > death[dead]).all()
    gone = np.asarray(leaves) == 0          # colours that never were: (0, ALIVE, 0, 0)
    gone[0] = False
    assert (~dead[gone]).all() and (np.asarray(area)[gone] == 0).all()
    assert (np.asarray(leaves)[dead] >= 1).all() and (np.asarray(area)[dead] >= 1).all()
    if vals is not None:
        for L in range(vals.shape[0]):
            r = roots_at(parent, death, L)
            assert (r[ex] == vals[L][ex]).all(), L
