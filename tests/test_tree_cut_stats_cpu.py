"""tree_cut with catalogue thresholds on the CPU: on every case the GPU tests use the two derivations of tests/tree_cut_stats_ref.py
agree and the five quantities of the keep test are monotone along `parent`; the cases reach the regimes they are there for
(conditions on the oracle's records, not measurements); the 64-bit cases are in their regime; a foreign catalogue is not monotone,
which is what makes table-then-walk the definition; and the host-side pieces of the bindings are in order."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import tree_cut_ref as tc
import tree_cut_stats_ref as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.mark.parametrize("name", ts.ALL)
def test_walk_equals_the_restatement_from_the_planes(name):
    f, cuts = ts.cuts_of(name)
    for cut in cuts:
        assert (f.cut(cut) == f.cut_planes(cut)).all(), (name, cut)
        if not cut.catalogue:      # ... and without catalogue thresholds both are tree_cut_ref's
            assert (f.cut(cut) == f.f.cut(cut.plain())).all(), (name, cut)


@pytest.mark.parametrize("name", ts.ALL)
def test_the_five_quantities_are_monotone_along_parent(name):
    f = ts.field(name)
    q = ts.quantities(f.death, f.area, f.leaves, f.stats)
    dead = np.flatnonzero(f.death != ts.ALIVE)
    up = f.parent[dead]
    assert dead.size and (f.death[up] > f.death[dead]).all()
    for k in ("area", "leaves", "sum_w", "w_max"):
        assert (q[k][up] >= q[k][dead]).all(), (name, k)
    assert (f.stats["w_min"][up] <= f.stats["w_min"][dead]).all(), name
    both = dead[f.death[up] != ts.ALIVE]      # the depth of an alive node is 0 by definition, and it is kept anyway
    assert (q["depth"][f.parent[both]] >= q["depth"][both]).all(), name


# ---- the regimes ------------------------------------------------------------------------------------------------------------------

def _moved(f, cut):
    return f.table(cut) != np.arange(f.n_seeds + 1)


@pytest.mark.parametrize("name", ["random48x52", "random40x37_edge", "walls", "plateau"])
def test_each_threshold_moves_entries_no_plain_cut_of_the_call_moves(name):
    f, cuts = ts.cuts_of(name)
    plain = np.zeros(f.n_seeds + 1, dtype=bool)
    for cut in cuts:
        if not cut.catalogue:
            plain |= _moved(f, cut)
    assert plain.any()      # the call has plain cuts that move something
    seen = set()
    for cut in cuts:
        if cut.catalogue and not (cut.min_area or cut.min_leaves) and (_moved(f, cut) & ~plain).any():
            seen |= {k for k in ("min_sum_w", "min_w_max", "min_depth") if getattr(cut, k)}
    want = {"random48x52": {"min_sum_w", "min_w_max", "min_depth"}, "random40x37_edge": {"min_sum_w", "min_w_max", "min_depth"},
            "walls": {"min_w_max", "min_depth"}, "plateau": {"min_sum_w", "min_depth"}}[name]
    assert want <= seen, (name, seen)


@pytest.mark.parametrize("name", sorted(ts.EXACT))
def test_a_threshold_is_met_exactly_and_one_more_drops_the_node(name):
    f, cuts = ts.cuts_of(name)
    keys = {c.key() for c in cuts}
    q = ts.quantities(f.death, f.area, f.leaves, f.stats)
    dead = f.death != ts.ALIVE
    for what, v in ts.EXACT[name]:
        at, above = ts.Cut(**{"min_" + what: v}), ts.Cut(**{"min_" + what: v + 1})
        assert at.key() in keys and above.key() in keys, (name, what)      # both are cuts of the case
        on = dead & (q[what] == v)
        assert on.any(), (name, what, v)
        assert f.keep(at)[on].all() and not f.keep(above)[on].any(), (name, what, v)
        assert (f.table(at) != f.table(above)).any(), (name, what, v)
        if name != "adjacent":      # (a node that dies at level 0 is left by every pixel's walk: only the tables differ)
            assert (f.cut(at) != f.cut(above)).any(), (name, what, v)
    if name == "walls":
        assert int((dead & (q["depth"] == 17)).sum()) == 32


def test_a_seed_alone_dies_at_level_zero_with_depth_clamped_to_zero():
    f, cuts = ts.cuts_of("adjacent")
    assert f.death[2] == 0 and f.area[2] == 1 and f.parent[2] == 1
    assert int(f.stats["w_min"][2]) == 3 and int(f.stats["sum_w"][2]) == 3      # death_level < w_min: the depth clamps
    assert ts.depth_of(f.death, f.stats["w_min"])[2] == 0
    assert f.table(ts.Cut(min_sum_w=3))[2] == 2 and f.table(ts.Cut(min_sum_w=4))[2] == 1 and f.table(ts.Cut(min_depth=1))[2] == 1
    assert {c.key() for c in (ts.Cut(min_sum_w=3), ts.Cut(min_sum_w=4), ts.Cut(min_depth=1))} <= {c.key() for c in cuts}


def test_thresholds_combine_with_the_levels():
    f, cuts = ts.cuts_of("random48x52")
    cut = ts.Cut(min_depth=87, show_level=200, merge_level=60)
    assert cut.key() in {c.key() for c in cuts}
    got = f.cut(cut)
    t = tc.levels_of(f.keys)
    assert ((got == 0) == ((f.seg == 0) | (t > 200))).all() and (t > 200).any()
    assert (got != f.cut(ts.Cut(min_depth=87, merge_level=60))).any()      # the show level matters
    assert (got != f.f.cut(tc.Cut(show_level=200, merge_level=60))).any()      # ... and so does the threshold
    g, gcuts = ts.cuts_of("random40x37_edge")
    both = ts.Cut(min_depth=20, merge_level=40)
    assert both.key() in {c.key() for c in gcuts}
    assert (g.cut(both) != g.cut(ts.Cut(min_depth=20))).any() and (g.cut(both) != g.cut(ts.Cut(merge_level=40))).any()


def test_a_huge_sum_drops_every_dead_node():
    f = ts.field("random48x52")
    dead = f.death != ts.ALIVE
    assert int(dead.sum()) == 257
    plane = f.cut(ts.Cut(min_sum_w=10 ** 12))
    lakes = np.unique(plane)      # two values: the hidden pixels and the one lake that never died
    assert lakes.size == 2 and lakes[0] == 0 and f.death[lakes[1]] == ts.ALIVE


def test_every_cut_is_nontrivial():
    # (adjacent: its only dead node dies at level 0 and every pixel's walk leaves it, the test above holds its tables; the 64-bit
    # cases hold thresholds that must KEEP a node, below)
    for name in ("random48x52", "random40x37_edge", "random40x37_edge_shift", "walls", "plateau"):
        f, cuts = ts.cuts_of(name)
        for cut in cuts:
            if cut.catalogue and not cut.min_leaves:      # (the cuts with min_leaves are there for the mix of thresholds)
                assert (f.cut(cut) != f.f.cut(cut.plain())).any(), (name, cut)


# ---- 64-bit sums --------------------------------------------------------------------------------------------------------------------

def test_staircase_sums_stay_below_two_to_the_32():
    f = ts.field("staircase_u16max")
    dead = f.death != ts.ALIVE
    s = f.stats["sum_w"]
    assert int(dead.sum()) == 254 and int(s[dead].max()) == ts.STAIR_TOP < 1 << 32
    # a compare that drops the high word of 2^32 + 5 would test against 5 and keep every node
    assert (s[dead] >= 5).all() and not f.keep(ts.Cut(min_sum_w=(1 << 32) + 5))[dead].any()
    assert int(f.keep(ts.Cut(min_sum_w=ts.STAIR_TOP))[dead].sum()) == 1 and not f.keep(ts.Cut(min_sum_w=ts.STAIR_TOP + 1))[dead].any()


def test_two_lakes_has_a_dead_lake_whose_sum_passes_two_to_the_32():
    f = ts.field("two_lakes_u16max")
    assert f.shape[0] <= 260 and f.shape[1] <= 260
    assert f.death[2] != ts.ALIVE and f.parent[2] == 1 and f.death[1] == ts.ALIVE
    assert int(f.area[2]) >= 65538
    s = int(f.stats["sum_w"][2])
    assert s == int(f.area[2]) * 65535 and s >= 1 << 32
    # the low word of the sum lies below the low word of 2^32 - 1: a 32-bit compare drops the node the 64-bit one keeps
    assert (s & 0xFFFFFFFF) < 0xFFFFFFFF
    assert f.keep(ts.Cut(min_sum_w=(1 << 32) - 1))[2] and f.keep(ts.Cut(min_sum_w=s))[2] and not f.keep(ts.Cut(min_sum_w=s + 1))[2]
    assert (f.cut(ts.Cut(min_sum_w=(1 << 32) - 1)) != f.cut(ts.Cut(min_sum_w=s + 1))).any()


# ---- a catalogue of another flood ---------------------------------------------------------------------------------------------------

def test_a_foreign_catalogue_is_not_monotone_and_the_table_is_still_defined():
    f, cuts = ts.cuts_of("random40x37")
    other = ts.foreign_catalogue()
    assert other.shape == f.stats.shape and (other["sum_w"] != f.stats["sum_w"]).any()
    dead = np.flatnonzero(f.death != ts.ALIVE)
    assert (other["sum_w"][f.parent[dead]] < other["sum_w"][dead]).any()
    differs = False
    for cut in cuts:
        got = f.cut_with(other, cut)
        assert got.shape == f.shape
        differs |= bool((got != f.cut(cut)).any())
    assert differs


# ---- the bindings' host side ----------------------------------------------------------------------------------------------------------

def test_cut_carries_the_catalogue_thresholds(pkg):
    c = pkg.Cut()
    assert (c.min_sum_w, c.min_w_max, c.min_depth) == (0, 0, 0) and not c.catalogue
    assert repr(c) == "Cut(min_area=0, min_leaves=0, show_level=254, merge_level=0)"
    d = pkg.Cut(3, 2, 10, 20, min_sum_w=(1 << 40) + 1, min_w_max=7, min_depth=9)
    assert d.catalogue and d != pkg.Cut(3, 2, 10, 20) and d == pkg.Cut(3, 2, 10, 20, (1 << 40) + 1, 7, 9) and "min_sum_w" in repr(d)
    for kw in ({"min_sum_w": -1}, {"min_sum_w": 1 << 64}, {"min_w_max": 1 << 32}, {"min_depth": -1}):
        with pytest.raises(ValueError):
            pkg.Cut(**kw)
    with pytest.raises(TypeError):
        pkg.Cut(min_depth=1.0)
    api = ge.load_package().api
    with pytest.raises(ValueError):      # the plain struct has no room for them
        api._as_cuts([d])
    arr, n = api._as_lake_cuts([d, c])
    assert n == 2 and (arr[0].min_sum_w, arr[0].min_area, arr[0].min_leaves, arr[0].min_w_max, arr[0].min_depth, arr[0].show_level,
                       arr[0].merge_level, list(arr[0].reserved)) == ((1 << 40) + 1, 3, 2, 7, 9, 10, 20, [0] * 6)
    L = pkg._ffi.LakeCut
    assert ctypes.sizeof(L) == 32 and (L.min_sum_w.offset, L.min_area.offset, L.min_leaves.offset, L.min_w_max.offset, L.min_depth.offset,
                                       L.show_level.offset, L.merge_level.offset, L.reserved.offset) == (0, 8, 12, 16, 20, 24, 25, 26)


@pytest.mark.parametrize("name", ["random48x52", "adjacent", "plateau", "staircase_u16max"])
def test_cut_table_against_the_reference(pkg, name):
    f, cuts = ts.cuts_of(name)
    tree = pkg.MergeTree(f.parent, f.death, f.area, f.leaves)
    for cut in cuts:
        got = tree.cut_table(pkg.Cut(*cut.key()), f.stats)
        assert got.dtype == np.uint32 and (got == f.table(cut)).all(), (name, cut)
    with pytest.raises(ValueError):
        tree.cut_table(pkg.Cut(min_depth=1))


def test_declarations_are_consistent(pkg):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ws_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "src", "hip_ffi.rs")).read()
    for name in ("ws_tree_cut_stats_device", "ws_merge_tree_stats_cut"):
        m = re.search(r"\bint %s\((.*?)\);" % name, header, flags=re.S)
        assert m, name
        n_args = len(m.group(1).split(","))
        assert n_args == len(pkg._ffi.SIGNATURES[name][1]), name
        r = re.search(r"pub fn %s\((.*?)\)\s*->\s*c_int;" % name, rust, flags=re.S)
        assert r and len([a for a in r.group(1).split(",") if a.strip()]) == n_args, name
    assert "typedef struct ws_lake_cut" in header and "pub struct ws_lake_cut" in rust
    assert getattr(ctypes.CDLL(pkg._ffi.LIB_PATH), "ws_tree_cut_stats_device") is not None
    assert getattr(ctypes.CDLL(pkg._ffi.LIB_PATH), "ws_merge_tree_stats_cut") is not None
