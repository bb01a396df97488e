"""tree_cut (ws_tree_cut_device, ws_merge_tree_cut) derived with numpy from the CPU oracle, twice: `cut_by_walk` follows the
definition of include/ws_hip.h (a table per cut, then a walk per pixel) over the tree of tests/merge_tree_ref.py and the oracle's
arrival stamps; `cut_by_planes` restates it from the oracle's per-level merging planes without any tree walk.  The cases the CPU
and GPU tests share are built here once per process and never changed afterwards."""
import numpy as np

import merge_tree_ref as mt
import merging_cases as mc
import oracle_lib as ol

ALIVE = mt.ALIVE
NEVER = (1 << 64) - 1      # the oracle's key of a pixel no level coloured


class Cut:
    """The four numbers of a cut, as plain data (the reference does not import the package)."""

    def __init__(self, min_area=0, min_leaves=0, show_level=254, merge_level=0):
        self.min_area, self.min_leaves, self.show_level, self.merge_level = int(min_area), int(min_leaves), int(show_level), int(merge_level)

    def key(self):
        return self.min_area, self.min_leaves, self.show_level, self.merge_level

    def __repr__(self):
        return "Cut(A=%d, K=%d, show=%d, merge=%d)" % self.key()


def kept(parent, death, area, leaves, cut):
    return (death == ALIVE) | ((area >= cut.min_area) & (leaves >= cut.min_leaves))


def cut_table(parent, death, area, leaves, cut):
    """T[c]: the first kept node of c's chain.  The cap is that of merge_tree_ref.roots_at."""
    keep = kept(parent, death, area, leaves, cut)
    node = np.arange(parent.size, dtype=np.int64)
    for _ in range(258):
        gone = ~keep[node]
        if not gone.any():
            return node
        node[gone] = parent[node[gone]]
    raise AssertionError("the parent walk does not end")


def levels_of(keys):
    """The arrival level of every pixel from the oracle's keys (level << 32 | ring); 255 where no level coloured it."""
    return np.where(keys == NEVER, 255, keys >> np.uint64(32)).astype(np.int64)


def cut_by_walk(parent, death, area, leaves, seg, keys, cut, want_steps=False):
    """The plane of one cut: table, then the walk while death <= max(t, merge_level).  want_steps: also the steps each pixel
    walked and whether its table entry moved."""
    T = cut_table(parent, death, area, leaves, cut)
    c = seg.astype(np.int64)
    t = levels_of(keys)
    shown = (c != 0) & (t <= cut.show_level)
    until = np.maximum(t, cut.merge_level)
    node = T[c]
    steps = np.zeros(c.shape, dtype=np.int64)
    for _ in range(258):
        go = shown & (death[node].astype(np.int64) <= until)
        if not go.any():
            break
        node[go] = parent[node[go]]
        steps[go] += 1
    else:
        raise AssertionError("the pixel walk does not end")
    out = np.where(shown, node, 0).astype(np.uint32)
    return (out, steps, (T[c] != c) & shown) if want_steps else out


def cut_by_planes(planes, death, area, leaves, seg, keys, cut):
    """The literal restatement from the per-level merging planes P_L: start at L = max(t, merge_level), look at P_L[p], and when
    that lake is not kept jump to its death level and look again.  (P_L[p] is a lake of level L: it dies after L or never; when
    it dies at level D it is no lake from D on, so the next lake that holds p is P_D[p].)"""
    stack = np.stack(planes).astype(np.int64)      # (levels, h, w)
    top = len(planes) - 1
    c = seg.astype(np.int64)
    t = levels_of(keys)
    shown = (c != 0) & (t <= cut.show_level)
    # above the last level nothing merges: the lake is the last plane's, which is alive there
    L = np.minimum(np.maximum(t, cut.merge_level), top)
    L[~shown] = 0
    rows, cols = np.indices(c.shape)
    keep = (death == ALIVE) | ((area >= cut.min_area) & (leaves >= cut.min_leaves))
    out = np.zeros(c.shape, dtype=np.int64)
    todo = shown.copy()
    for _ in range(258):
        if not todo.any():
            break
        lake = stack[L, rows, cols]
        assert (lake[todo] != 0).all(), "a shown pixel is uncoloured in the plane of its own level"
        done = todo & keep[lake]
        out[done] = lake[done]
        todo &= ~done
        L = np.where(todo, death[lake].astype(np.int64), L)
        assert (L[todo] <= top).all(), "a lake that is not kept never dies"
    else:
        raise AssertionError("the jumps do not end")
    return out.astype(np.uint32)


def lists_of(plane, n_seeds):
    """(colours ascending, their pixel counts, pixels equal to 0) of one plane."""
    cols, counts = np.unique(plane, return_counts=True)
    hidden = int(counts[0]) if cols.size and cols[0] == 0 else 0
    nz = cols != 0
    return cols[nz].astype(np.uint64), counts[nz].astype(np.uint64), hidden


def expected_lists(planes, n_seeds):
    """What ws_tree_cut_device writes for the planes of a call: (records (n, 2) u64, offsets (K + 1), hidden (K))."""
    recs, offsets, hidden = [], [0], []
    for p in planes:
        cols, counts, hid = lists_of(p, n_seeds)
        recs.append(np.stack([cols, counts], axis=1))
        offsets.append(offsets[-1] + len(cols))
        hidden.append(hid)
    rec = np.concatenate(recs) if recs else np.zeros((0, 2), dtype=np.uint64)
    return rec.reshape(-1, 2), np.array(offsets, dtype=np.uint64), np.array(hidden, dtype=np.uint64)


class Field:
    """One flood as the oracle sees it: the tree, the segmenting labels, the keys, the per-level planes; planes of cuts on demand."""

    def __init__(self, name, img, seeds, max_level=254, edge=False, seed_shift=False):
        self.name, self.img = name, np.ascontiguousarray(img, dtype=np.uint8)
        self.seeds = np.asarray(seeds, dtype=np.int64).reshape(-1, 2)
        self.max_level, self.edge, self.seed_shift = int(max_level), bool(edge), bool(seed_shift and edge)
        self.planes, self.ps = mt.oracle_planes(self.img, self.seeds, self.max_level, self.edge, self.seed_shift)
        self.parent, self.death, self.area, self.leaves, _, self.ex = mt.tree_from_planes(self.planes, self.ps)
        self.seg, self.keys = ol.segment_arrival(self.img, self.ps, max_level=self.max_level, edge=self.edge, want_keys=True)
        self.seg = self.seg.astype(np.uint32)
        self.tree = np.stack([self.parent, self.death, self.area, self.leaves], axis=1).astype(np.uint32)
        self.n_seeds = len(self.ps)
        self._cuts = {}

    @property
    def shape(self):
        return self.seg.shape

    def keys32(self):
        """The stamps as the engine holds them: level << 24 | ring, 0xFF000000 never coloured."""
        k = self.keys
        lvl, ring = k >> np.uint64(32), k & np.uint64(0xFFFFFFFF)
        return np.where(k == NEVER, 0xFF000000, (lvl << np.uint64(24)) | ring).astype(np.uint32)

    def cut(self, cut):
        hit = self._cuts.get(cut.key())
        if hit is None:
            hit = cut_by_walk(self.parent, self.death, self.area, self.leaves, self.seg, self.keys, cut)
            hit.setflags(write=False)
            self._cuts[cut.key()] = hit
        return hit

    def cut_planes(self, cut):
        return cut_by_planes(self.planes, self.death, self.area, self.leaves, self.seg, self.keys, cut)


_FIELDS = {}


def field(name):
    """The shared cases by name, built on first use."""
    if name not in _FIELDS:
        _FIELDS[name] = _BUILDERS[name]()
    return _FIELDS[name]


def _random(name, h, w, seed, **kw):
    img = ol.random_field(h, w, seed)
    return lambda: Field(name, img, ol.find_local_minima(img), **kw)


def _adjacent():
    """Two horizontally adjacent seeds on a floor, and a wall: the larger colour dies at level 0 with area 1."""
    img = np.full((9, 12), 3, dtype=np.uint8)
    img[:, 8] = 255
    return Field("adjacent", img, [(4, 3), (4, 4), (2, 10)])


def _from_case(case):
    return lambda: Field(case.name, case.img, case.seeds, case.max_level, case.edge, case.seed_shift)


def _small_merging(kind, form, h, w, n, seed, **kw):
    def make():
        rng = np.random.default_rng(seed)
        return Field(f"{kind}_{form}", mc.make_field(kind, h, w, rng), mc.make_seeds(form, h, w, n, rng), **kw)
    return make


_BUILDERS = {
    "random48x52": _random("random48x52", 48, 52, 1),
    "random40x37": _random("random40x37", 40, 37, 2, max_level=100),
    "random40x37_edge": _random("random40x37_edge", 40, 37, 2, max_level=100, edge=True),
    "random40x37_edge_shift": _random("random40x37_edge_shift", 40, 37, 2, max_level=100, edge=True, seed_shift=True),
    "random33x64": _random("random33x64", 33, 64, 3, max_level=100),
    "random257x4": _random("random257x4", 257, 4, 4),
    "random1x3": lambda: Field("random1x3", np.array([[5, 1, 7]], dtype=np.uint8), [(0, 1)]),
    "random3x1": lambda: Field("random3x1", np.array([[5], [1], [7]], dtype=np.uint8), [(1, 0)]),
    "adjacent": _adjacent,
    "staircase": _from_case(mc.staircase()),
    "plateau": _small_merging("few", "repeats", 30, 44, 90, 11),
    "walls": _small_merging("walls", "shuffled", 36, 40, 70, 12),
    "constant": _small_merging("constant", "borders", 20, 36, 40, 13, max_level=17),
}

# the nine cuts of the random 48 x 52 case, unsorted, one duplicate
RANDOM_CUTS = [Cut(min_area=16), Cut(show_level=254, merge_level=254), Cut(min_leaves=3), Cut(min_area=4), Cut(min_area=30, min_leaves=4),
               Cut(show_level=0, merge_level=0), Cut(min_area=10 ** 6), Cut(min_area=64), Cut(show_level=50, merge_level=50), Cut(min_area=16)]
NONTRIVIAL = [Cut(min_area=4), Cut(min_area=16), Cut(min_area=64), Cut(min_leaves=3), Cut(min_area=30, min_leaves=4)]
# cuts for the other fields: thresholds, both levels, and the two together
MIXED_CUTS = [Cut(), Cut(min_area=5), Cut(min_leaves=2, show_level=60), Cut(min_area=12, merge_level=40), Cut(show_level=30, merge_level=70),
              Cut(show_level=100, merge_level=100), Cut(min_area=7, min_leaves=2, show_level=80, merge_level=20)]


def staircase_cuts(f):
    """Around the mid-chain node of the 254-deep staircase: min_area just below, at and above its area; leaves; a merge level."""
    mid = 128
    a = int(f.area[mid])
    return [Cut(min_area=a - 1), Cut(min_area=a), Cut(min_area=a + 1), Cut(min_leaves=128), Cut(merge_level=127),
            Cut(min_area=a, show_level=200, merge_level=127)]
