"""tree_cut with catalogue thresholds (ws_tree_cut_stats_device, ws_merge_tree_stats_cut) derived with numpy from the CPU oracle,
twice, over the tree of tests/merge_tree_ref.py and the catalogue of tests/lake_stats_ref.py: `cut_by_walk` is the definition of
include/ws_hip.h (a table per cut, then a walk per pixel -- total for ANY catalogue), `cut_by_planes` restates it from the
oracle's per-level merging planes and never follows `parent` (equal to the walk for the catalogue of the tree's own flood).  The
cases the CPU and GPU tests share are built here once per process and never changed afterwards."""
import numpy as np

import lake_stats_ref as ls
import merging_cases as mc
import oracle_lib as ol
import tree_cut_ref as tc

ALIVE = tc.ALIVE


class Cut(tc.Cut):
    """The seven numbers of a cut, as plain data."""

    def __init__(self, min_area=0, min_leaves=0, show_level=254, merge_level=0, min_sum_w=0, min_w_max=0, min_depth=0):
        super().__init__(min_area, min_leaves, show_level, merge_level)
        self.min_sum_w, self.min_w_max, self.min_depth = int(min_sum_w), int(min_w_max), int(min_depth)

    def key(self):
        return super().key() + (self.min_sum_w, self.min_w_max, self.min_depth)

    @property
    def catalogue(self):
        return bool(self.min_sum_w or self.min_w_max or self.min_depth)

    def plain(self):
        """The cut without its catalogue thresholds."""
        return tc.Cut(self.min_area, self.min_leaves, self.show_level, self.merge_level)

    def __repr__(self):
        return "Cut(A=%d, K=%d, show=%d, merge=%d, S=%d, P=%d, D=%d)" % self.key()


def depth_of(death, w_min):
    """death_level - w_min where the node died above its smallest weight, else 0."""
    d, m = death.astype(np.int64), w_min.astype(np.int64)
    return np.where((death != ALIVE) & (d > m), d - m, 0)


def quantities(death, area, leaves, stats):
    """The five quantities of the keep test, per node: area, n_leaves, sum_w (uint64), w_max, depth."""
    return {"area": area.astype(np.int64), "leaves": leaves.astype(np.int64), "sum_w": stats["sum_w"].astype(np.uint64),
            "w_max": stats["w_max"].astype(np.int64), "depth": depth_of(death, stats["w_min"])}


def kept(death, area, leaves, stats, cut):
    q = quantities(death, area, leaves, stats)
    return (death == ALIVE) | ((q["area"] >= cut.min_area) & (q["leaves"] >= cut.min_leaves) & (q["sum_w"] >= np.uint64(cut.min_sum_w)) &
                               (q["w_max"] >= cut.min_w_max) & (q["depth"] >= cut.min_depth))


def cut_table(parent, keep):
    """T[c]: the first kept node of c's chain (an alive node is kept)."""
    node = np.arange(parent.size, dtype=np.int64)
    for _ in range(258):
        gone = ~keep[node]
        if not gone.any():
            return node
        node[gone] = parent[node[gone]]
    raise AssertionError("the parent walk does not end")


def cut_by_walk(parent, death, keep, seg, keys, cut):
    """Table, then the walk while death <= max(t, merge_level)."""
    T = cut_table(parent, keep)
    c = seg.astype(np.int64)
    t = tc.levels_of(keys)
    shown = (c != 0) & (t <= cut.show_level)
    until = np.maximum(t, cut.merge_level)
    node = T[c]
    for _ in range(258):
        go = shown & (death[node].astype(np.int64) <= until)
        if not go.any():
            break
        node[go] = parent[node[go]]
    else:
        raise AssertionError("the pixel walk does not end")
    return np.where(shown, node, 0).astype(np.uint32)


def cut_by_planes(planes, death, keep, seg, keys, cut):
    """From the per-level merging planes P_L alone: start at L = max(t, merge_level), look at P_L[p], and when that lake is not kept
    jump to its death level and look again (tree_cut_ref.cut_by_planes with another keep test)."""
    stack = np.stack(planes).astype(np.int64)
    top = len(planes) - 1
    c = seg.astype(np.int64)
    t = tc.levels_of(keys)
    shown = (c != 0) & (t <= cut.show_level)
    L = np.minimum(np.maximum(t, cut.merge_level), top)
    L[~shown] = 0
    rows, cols = np.indices(c.shape)
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


class Field:
    """A flood of tree_cut_ref with a weight plane (None: the image) and the catalogue of its lakes."""

    def __init__(self, name, f, weights=None):
        self.name, self.f, self.weights = name, f, weights
        self.stats = ls.stats_from_planes(f.planes, f.ps, ls.plane_weights(f.img, weights, f.edge), f.death, f.ex)
        self.stats.setflags(write=False)
        self._cuts = {}

    def __getattr__(self, k):      # the flood's own attributes: img, seeds, tree, seg, keys, planes, n_seeds, shape, edge ...
        return getattr(self.f, k)

    def keep(self, cut, stats=None):
        f = self.f
        return kept(f.death, f.area, f.leaves, self.stats if stats is None else stats, cut)

    def cut(self, cut):
        hit = self._cuts.get(cut.key())
        if hit is None:
            f = self.f
            hit = cut_by_walk(f.parent, f.death, self.keep(cut), f.seg, f.keys, cut)
            hit.setflags(write=False)
            self._cuts[cut.key()] = hit
        return hit

    def cut_with(self, stats, cut):
        """Table then walk with a catalogue that need not belong to the tree."""
        f = self.f
        return cut_by_walk(f.parent, f.death, self.keep(cut, stats), f.seg, f.keys, cut)

    def cut_planes(self, cut):
        f = self.f
        return cut_by_planes(f.planes, f.death, self.keep(cut), f.seg, f.keys, cut)

    def table(self, cut):
        return cut_table(self.f.parent, self.keep(cut))


def _two_lakes():
    """260 x 260 at value 0 with one column of value 2: seed 1 in the single column right of it, seed 2 on the 258 columns left of
    it.  The barrier floods at level 2 and the larger colour dies with 66306 pixels (the outer ring of a plane is never flooded)."""
    img = np.zeros((260, 260), dtype=np.uint8)
    img[:, 258] = 2
    return tc.Field("two_lakes", img, [(5, 259), (100, 100)], max_level=3)


def _u16max(f):
    return np.full(f.img.shape, 65535, dtype=np.uint16)


_FIELDS = {}
_BUILDERS = {
    "random48x52": lambda: Field("random48x52", tc.field("random48x52")),
    "random48x52_u16": lambda: Field("random48x52_u16", tc.field("random48x52"), mc.weight_planes((48, 52), 1)[2][1]),
    "random40x37": lambda: Field("random40x37", tc.field("random40x37")),
    "random40x37_edge": lambda: Field("random40x37_edge", tc.field("random40x37_edge")),
    "random40x37_edge_shift": lambda: Field("random40x37_edge_shift", tc.field("random40x37_edge_shift")),
    "walls": lambda: Field("walls", tc.field("walls")),
    "plateau": lambda: Field("plateau", tc.field("plateau")),
    "adjacent": lambda: Field("adjacent", tc.field("adjacent")),
    "staircase_u16max": lambda: Field("staircase_u16max", tc.field("staircase"), _u16max(tc.field("staircase"))),
    "two_lakes_u16max": lambda: (lambda f: Field("two_lakes_u16max", f, _u16max(f)))(_two_lakes()),
}


def field(name):
    """The shared cases by name, built on first use."""
    if name not in _FIELDS:
        _FIELDS[name] = _BUILDERS[name]()
    return _FIELDS[name]


def foreign_catalogue():
    """The catalogue of ANOTHER random 40 x 37 field, cut or repeated to the record count of random40x37's tree."""
    if "foreign" not in _FIELDS:
        img = ol.random_field(40, 37, 9)
        other = Field("other40x37", tc.Field("other40x37", img, ol.find_local_minima(img), max_level=100))
        _FIELDS["foreign"] = np.resize(other.stats, field("random40x37").n_seeds + 1)
        _FIELDS["foreign"].setflags(write=False)
    return _FIELDS["foreign"]


# ---- the cuts of every case: thresholds in pairs stand just at and just above a node's value -----------------------------------------
# (the plain cuts travel in the same call: the regimes compare the catalogue tables with theirs, so they are mild ones -- min_leaves
# = 2 alone moves every leaf, which is most of a tree)
CUTS = {
    "random48x52": [Cut(min_sum_w=336), Cut(min_depth=55), Cut(min_area=4), Cut(min_w_max=240), Cut(min_sum_w=335), Cut(min_depth=56),
                    Cut(min_w_max=239), Cut(min_sum_w=893, min_depth=30), Cut(), Cut(min_depth=87, show_level=200, merge_level=60),
                    Cut(min_w_max=250, min_area=4), Cut(min_sum_w=10 ** 12), Cut(min_area=2, min_leaves=1), Cut(min_depth=55),
                    Cut(min_w_max=240, min_leaves=2, merge_level=30), Cut(min_area=4)],
    "random40x37_edge": [Cut(min_sum_w=223), Cut(min_area=4), Cut(min_depth=48), Cut(), Cut(min_w_max=147), Cut(min_depth=20, merge_level=40),
                         Cut(min_area=2, min_leaves=1), Cut(min_w_max=147, min_leaves=2, show_level=60)],
    "walls": [Cut(min_depth=18), Cut(min_area=4), Cut(min_depth=17), Cut(min_w_max=200), Cut(), Cut(min_area=2, min_leaves=1)],
    "plateau": [Cut(min_depth=80), Cut(min_sum_w=160), Cut(min_area=4), Cut(min_depth=81), Cut(), Cut(min_area=2, min_leaves=1)],
    "adjacent": [Cut(min_sum_w=4), Cut(min_sum_w=3), Cut(min_depth=1), Cut(), Cut(min_area=4)],
}
CUTS["random40x37_edge_shift"] = CUTS["random40x37_edge"]
CUTS["random40x37"] = CUTS["random40x37_edge"]
# (threshold, threshold + 1) pairs that a dead node of the case meets exactly, by quantity
EXACT = {
    "random48x52": [("sum_w", 335), ("depth", 55), ("w_max", 239)],
    "walls": [("depth", 17)],
    "plateau": [("depth", 80)],
    "adjacent": [("sum_w", 3)],
}

STAIR_TOP = 4277797125            # the largest dead sum_w of the staircase under weights of 65535: below 2^32
STAIR_CUTS = [Cut(min_sum_w=(1 << 32) + 5), Cut(min_sum_w=STAIR_TOP), Cut(), Cut(min_sum_w=STAIR_TOP + 1), Cut(min_sum_w=65535 * 30000, merge_level=10)]


def two_lakes_cuts(f):
    """Around the dead lake's sum, which lies above 2^32."""
    s = int(f.stats["sum_w"][2])
    return [Cut(min_sum_w=(1 << 32) - 1), Cut(min_sum_w=s + 1), Cut(min_sum_w=s), Cut(), Cut(min_sum_w=1 << 32)]


def u16_cuts(f):
    """For the u16 weight plane of the random field: thresholds at quantiles of the dead nodes' own values."""
    dead = f.death != ALIVE
    q = quantities(f.death, f.area, f.leaves, f.stats)
    s = np.sort(q["sum_w"][dead])
    p = np.sort(q["w_max"][dead])
    return [Cut(min_sum_w=int(s[len(s) // 2])), Cut(min_w_max=int(p[len(p) // 2])), Cut(min_area=4), Cut(min_sum_w=int(s[len(s) // 2]) + 1),
            Cut(min_sum_w=int(s[3 * len(s) // 4]), min_w_max=int(p[len(p) // 4]), show_level=180, merge_level=90), Cut(), Cut(min_depth=1)]


def cuts_of(name):
    f = field(name)
    if name == "staircase_u16max":
        return f, STAIR_CUTS
    if name == "two_lakes_u16max":
        return f, two_lakes_cuts(f)
    if name == "random48x52_u16":
        return f, u16_cuts(f)
    return f, CUTS[name]


ALL = ["random48x52", "random48x52_u16", "random40x37", "random40x37_edge", "random40x37_edge_shift", "walls", "plateau", "adjacent",
       "staircase_u16max", "two_lakes_u16max"]
