"""tree_cut on the CPU: the two derivations of tests/tree_cut_ref.py agree on every case the GPU tests use, the level cuts are
the merging history planes, the cases reach the regimes they are there for (conditions on the oracle's records, not
measurements), and the host-side pieces of the bindings -- Cut, MergeTree.cut_table, the declarations -- are in order."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import merge_tree_ref as mt
import tree_cut_ref as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


def _cuts_of(name):
    f = tc.field(name)
    if name == "random48x52":
        return f, tc.RANDOM_CUTS
    if name == "staircase":
        return f, tc.staircase_cuts(f)
    return f, tc.MIXED_CUTS


SMALL = ["random48x52", "random40x37", "random40x37_edge", "random40x37_edge_shift", "random33x64", "random257x4", "random1x3",
         "random3x1", "adjacent", "plateau", "walls", "constant"]


@pytest.mark.parametrize("name", SMALL + ["staircase"])
def test_walk_equals_the_restatement_from_the_planes(name):
    f, cuts = _cuts_of(name)
    mt.check_invariants(f.parent, f.death, f.area, f.leaves)
    for cut in cuts:
        assert (f.cut(cut) == f.cut_planes(cut)).all(), (name, cut)


@pytest.mark.parametrize("name", ["random48x52", "random40x37_edge", "walls", "constant"])
def test_level_cut_is_the_history_plane(name):
    f = tc.field(name)
    for L in sorted({0, 1, 17, 50, f.max_level}):
        if L <= f.max_level:
            assert (f.cut(tc.Cut(show_level=L, merge_level=L)) == f.planes[L]).all(), (name, L)


def test_area_and_leaves_grow_along_parent():
    # what makes the two climbs commute: with death levels (check_invariants), areas and leaves strictly increase up the chain
    for name in SMALL + ["staircase"]:
        f = tc.field(name)
        dead = np.flatnonzero(f.death != tc.ALIVE)
        assert (f.area[f.parent[dead]] > f.area[dead]).all() and (f.leaves[f.parent[dead]] > f.leaves[dead]).all(), name


def test_lists_add_up():
    for name in SMALL:
        f, cuts = _cuts_of(name)
        rec, offsets, hidden = tc.expected_lists([f.cut(c) for c in cuts], f.n_seeds)
        for k in range(len(cuts)):
            part = rec[int(offsets[k]): int(offsets[k + 1])]
            assert (np.diff(part[:, 0].astype(np.int64)) > 0).all()
            assert int(hidden[k]) + int(part[:, 1].sum()) == f.seg.size


# ---- the regimes ------------------------------------------------------------------------------------------------------------------

def test_random_case_figures():
    f = tc.field("random48x52")
    assert f.n_seeds == 258 and int((f.ex[1:] & (f.death[1:] == tc.ALIVE)).sum()) == 1
    regions = {c.key(): int(np.unique(f.cut(c)[f.cut(c) != 0]).size) for c in tc.NONTRIVIAL}
    assert [regions[c.key()] for c in tc.NONTRIVIAL[:4]] == [129, 47, 17, 63]


def test_nontrivial_cuts_lie_between_roots_and_colours():
    f = tc.field("random48x52")
    roots = int((f.ex[1:] & (f.death[1:] == tc.ALIVE)).sum())
    colours = int(f.ex[1:].sum())
    for cut in tc.NONTRIVIAL:
        regions = np.unique(f.cut(cut))
        n = int((regions != 0).sum())
        assert roots < n < colours, (cut, roots, n, colours)


def test_table_and_walk_move_alone_and_together():
    f = tc.field("random48x52")
    seen = set()
    for cut in tc.RANDOM_CUTS:
        _, steps, moved = tc.cut_by_walk(f.parent, f.death, f.area, f.leaves, f.seg, f.keys, cut, want_steps=True)
        shown = (f.seg != 0) & (tc.levels_of(f.keys) <= cut.show_level)
        seen |= {"table": bool((moved & (steps == 0)).any()), "walk": bool((shown & ~moved & (steps >= 1)).any()),
                 "both": bool((moved & (steps >= 1)).any())}.items()
    assert {("table", True), ("walk", True), ("both", True)} <= seen


def test_a_threshold_meets_an_area_exactly():
    f = tc.field("random48x52")
    dead = f.death != tc.ALIVE
    for a in (4, 16, 64):
        assert (f.area[dead] == a).any(), a          # >= decides these nodes
    s = tc.field("staircase")
    assert tc.staircase_cuts(s)[1].min_area == int(s.area[128]) and s.death[128] != tc.ALIVE


def test_adjacent_seeds_die_at_level_zero():
    f = tc.field("adjacent")
    assert f.death[2] == 0 and f.area[2] == 1 and f.parent[2] == 1
    T1 = tc.cut_table(f.parent, f.death, f.area, f.leaves, tc.Cut(min_area=1))
    T2 = tc.cut_table(f.parent, f.death, f.area, f.leaves, tc.Cut(min_area=2))
    assert T1[2] == 2 and T2[2] == 1


def test_some_pixel_is_never_coloured():
    for name in ("random40x37", "random33x64", "walls", "adjacent"):
        f = tc.field(name)
        assert (f.keys == tc.NEVER).any() and (f.keys32() == 0xFF000000).any(), name
    f = tc.field("random40x37")
    assert int((f.ex[1:] & (f.death[1:] == tc.ALIVE)).sum()) > 1


def test_nonexistent_colours_and_walls():
    f = tc.field("plateau")
    gone = ~f.ex[1:]
    assert gone.any() and (f.tree[1:][gone] == np.array([0, tc.ALIVE, 0, 0], dtype=np.uint32)).all()
    assert (tc.field("walls").img == 255).any()


def test_staircase_chain_is_254_deep():
    f = tc.field("staircase")
    depth, c = 0, f.n_seeds
    while f.death[c] != tc.ALIVE:
        c, depth = int(f.parent[c]), depth + 1
    assert depth == 254


# ---- the bindings' host side ----------------------------------------------------------------------------------------------------------

def test_cut_validation(pkg):
    c = pkg.Cut()
    assert (c.min_area, c.min_leaves, c.show_level, c.merge_level) == (0, 0, 254, 0)
    assert pkg.Cut(3, 2, 10, 20) == pkg.Cut(min_area=3, min_leaves=2, show_level=10, merge_level=20)
    for kw in ({"show_level": 255}, {"merge_level": 255}, {"min_area": -1}, {"min_leaves": 1 << 32}, {"show_level": -1}):
        with pytest.raises(ValueError):
            pkg.Cut(**kw)
    for kw in ({"min_area": 1.5}, {"show_level": "3"}, {"merge_level": True}):
        with pytest.raises(TypeError):
            pkg.Cut(**kw)
    with pytest.raises(AttributeError):
        c.min_area = 4
    api = ge.load_package().api
    with pytest.raises(ValueError):
        api._as_cuts([pkg.Cut()] * 33)
    with pytest.raises(TypeError):
        api._as_cuts([(0, 0, 254, 0)])
    arr, n = api._as_cuts([pkg.Cut(7, 2, 100, 50)])
    assert n == 1 and (arr[0].min_area, arr[0].min_leaves, arr[0].show_level, arr[0].merge_level, list(arr[0].reserved)) == (7, 2, 100, 50, [0, 0])
    assert ctypes.sizeof(pkg._ffi.TreeCut) == 12 and pkg._ffi.TreeCut.show_level.offset == 8 and pkg._ffi.TreeCut.merge_level.offset == 9


@pytest.mark.parametrize("name", ["random48x52", "adjacent", "plateau", "staircase"])
def test_cut_table_against_the_reference(pkg, name):
    f, cuts = _cuts_of(name)
    tree = pkg.MergeTree(f.parent, f.death, f.area, f.leaves)
    for cut in cuts:
        want = tc.cut_table(f.parent, f.death, f.area, f.leaves, cut)
        got = tree.cut_table(pkg.Cut(cut.min_area, cut.min_leaves, cut.show_level, cut.merge_level))
        assert got.dtype == np.uint32 and (got == want).all(), (name, cut)


def test_declarations_are_consistent(pkg):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ws_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "src", "hip_ffi.rs")).read()
    for name in ("ws_tree_cut_device", "ws_merge_tree_cut"):
        m = re.search(r"\bint %s\((.*?)\);" % name, header, flags=re.S)
        assert m, name
        n_args = len(m.group(1).split(","))
        assert n_args == len(pkg._ffi.SIGNATURES[name][1]), name
        r = re.search(r"pub fn %s\((.*?)\)\s*->\s*c_int;" % name, rust, flags=re.S)
        assert r and len([a for a in r.group(1).split(",") if a.strip()]) == n_args, name
    assert "typedef struct ws_tree_cut" in header and "pub struct ws_tree_cut" in rust
    assert getattr(ctypes.CDLL(pkg._ffi.LIB_PATH), "ws_tree_cut_device") is not None
