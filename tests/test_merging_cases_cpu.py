"""The generators of tests/merging_cases.py without a GPU: the CPU oracle's own records prove that the inputs reach the regimes
tests/test_gpu_merging_products_random.py is there for -- long parent chains, a thousand and more unions in one level, lakes of
many tiles, mass deaths at level 0, colours that do not exist, walls that keep a seed alone -- and every expected tree holds
the invariants of its definition."""
import numpy as np
import pytest

import merge_tree_ref as mt
import merging_cases as mc


@pytest.fixture(scope="module")
def sweep():
    cases = mc.sweep_cases()
    return [(c, mc.expected(c, want_stats=False, want_segmenting=False)) for c in cases]


@pytest.fixture(scope="module")
def constructed():
    return {c.name: (c, mc.expected(c, want_stats=False, want_segmenting=False)) for c in mc.constructed_cases()}


def _rows(pairs):
    return [mc.describe(c, e) for c, e in pairs]


def test_every_expected_tree_holds_the_invariants(sweep, constructed):
    for c, e in sweep + list(constructed.values()):
        mt.check_invariants(e.parent, e.death, e.area, e.leaves, e.vals, e.ex)
        alive = (e.death == mt.ALIVE) & e.ex
        ph, pw = c.plane_shape
        assert int(e.area[alive].sum()) + int(e.area[0]) == ph * pw, c
        assert int(e.leaves[alive].sum()) == int(e.ex.sum()), c
        assert e.labels.shape == (ph, pw) and len(e.lakes) == c.max_level + 1, c
        # the lake records of the last level are the survivors
        assert (e.lakes[-1][0] == np.flatnonzero(alive)).all() and (e.lakes[-1][1] == e.area[alive]).all(), c


def test_every_expected_tree_of_the_cubes_holds_the_invariants():
    for slices, _ in mc.cube_cases():
        for c in slices:
            e = mc.expected(c, want_stats=False, want_segmenting=False)
            mt.check_invariants(e.parent, e.death, e.area, e.leaves, e.vals, e.ex)
            assert (len(c.seeds) == 0) == (int(e.area[0]) == c.plane_shape[0] * c.plane_shape[1]), c


def test_constructed_cases_ask_for_every_level(constructed):
    for c, e in constructed.values():
        assert c.levels == list(range(c.max_level + 1)) and sorted(e.planes) == c.levels, c


def test_sweep_reaches_the_regimes(sweep):
    rows = _rows(sweep)
    assert sum(r["most_deaths"] >= 1000 for r in rows) >= 3                 # thousands of unions race in one launch
    assert sum(r["largest_lake"] >= 65536 for r in rows) >= 3               # lakes of four and more tiles of 256 x 64
    assert sum(r["deaths_at_0"] >= 1000 for r in rows) >= 1                 # mass deaths at level 0
    assert sum(r["nonexistent"] >= 100 for r in rows) >= 1                  # duplicate seeds: colours that never were
    assert sum(r["survivors_on_255_area_1"] >= 1 for r in rows) >= 1        # a seed on a wall stays alone
    assert sum(r["survivors"] >= 2 for r in rows) >= 2


def test_sweep_draws_every_kind_form_option_and_store_path(sweep):
    cases = [c for c, _ in sweep]
    assert 8 <= len(cases) <= 12
    assert {c.kind for c in cases} == set(mc.KINDS) and {c.form for c in cases} == set(mc.FORMS)
    assert {c.max_level for c in cases} == {254, 100, 17, 1}
    assert {(c.edge, c.seed_shift) for c in cases} == {(False, False), (True, False), (True, True)}
    widths = [c.img.shape[1] for c in cases]
    assert all((w % 4 != 0) == (i % 4 == 3) for i, w in enumerate(widths)), widths
    px = [c.plane_shape[0] * c.plane_shape[1] for c in cases]
    assert any(p % 2 == 1 for p in px) and any(p % 4 == 0 for p in px)      # the scalar stores of the history render, and the 16-byte ones
    assert all(3 <= c.img.shape[0] <= 330 and c.img.shape[1] <= 800 for c in cases)
    assert max(c.img.shape[0] for c in cases) > 256 and max(widths) > 4 * 128      # more than one tile both ways, ragged last tiles
    for c in cases:
        lv = c.levels
        assert 0 in lv and c.max_level in lv and len(set(lv)) < len(lv) and lv != sorted(lv), (c, lv)
    for c in cases:      # the forms are what they say
        flat = c.seeds[:, 0] * c.img.shape[1] + c.seeds[:, 1]
        increasing = bool((np.diff(flat) > 0).all())
        assert increasing == (c.form in ("sorted", "borders")), c
        if c.form == "repeats":
            assert len(np.unique(flat)) < len(flat)
        if c.form == "borders":
            h, w = c.img.shape
            assert {0, w - 1, (h - 1) * w, h * w - 1} <= set(flat.tolist())
            assert (np.diff(flat) == 1).any() and np.isin(flat + w, flat).any()


def test_staircase_is_a_chain_254_deep(constructed):
    c, e = constructed["staircase"]
    d = mc.describe(c, e)
    assert d["depth"] >= 200 and d["depth"] == 254 and d["survivors"] == 1 and d["largest_lake"] == 65790
    n = len(c.seeds)
    assert (e.parent[2:] == np.arange(1, n)).all() and e.parent[1] == 0
    # one colour dies per level: row c floods at level 255 - c, touches the seed pixel of row c - 1 above it and takes its colour
    assert (e.death[2:] == 255 - np.arange(2, n + 1)).all() and e.death[1] == mt.ALIVE
    # the walk of roots_at ends within its cap: death levels strictly increase along `parent`, so no chain exceeds 255 hooks
    assert (mt.roots_at(e.parent, e.death, 254)[1:] == 1).all()
    assert (mt.roots_at(e.parent, e.death, 100)[1:] == np.minimum(np.arange(1, n + 1), 154)).all()


def test_seeded_plateaus_die_at_level_zero(constructed):
    for name in ("plateau_w516", "plateau_w517"):
        c, e = constructed[name]
        at0 = e.death == 0
        assert at0.sum() >= 20000 and (e.area[at0] == 1).all() and (e.leaves[at0] == 1).all(), name
        assert c.img.shape[1] % 3 == (0 if name.endswith("516") else 1)
    c, _ = constructed["plateau_w516"]
    assert (c.seeds[:, 1] % 3 == 0).all()                                    # stacked in columns
    c, _ = constructed["plateau_w517"]
    assert len(np.unique(c.seeds[:, 1] % 3)) == 3


def test_two_seas_merge_exactly_from_v_on(constructed):
    v = mc.TWO_SEAS_V
    below, at, full = (constructed[f"two_seas_max{m}"][1] for m in (v - 1, v, 254))
    alive = lambda e: np.flatnonzero((e.death == mt.ALIVE) & e.ex)
    assert alive(below).size == 2 and alive(at).size == 1 and alive(full).size == 1      # levels are inclusive
    a, b = alive(below)
    assert min(below.area[a], below.area[b]) >= 65536                                    # two lakes of many tiles each
    assert at.death[b] == v and at.parent[b] == a and full.death[b] == v
    assert at.area[a] == below.area[a] + below.area[b] + 1                               # ... and the pixel between them
    assert (at.tree == full.tree).all()


def test_cubes_are_what_the_plan_says():
    cubes = mc.cube_cases()
    assert 8 <= len(cubes) <= 12
    stacks = []
    for slices, limit in cubes:
        assert 3 <= len(slices) <= 6
        assert sum(len(c.seeds) == 0 for c in slices) == 1                  # one seedless slice
        ph, pw = slices[0].plane_shape
        assert all(c.plane_shape == (ph, pw) and c.max_level == slices[0].max_level and c.edge == slices[0].edge for c in slices)
        stacks.append(pw % 4 == 0 and ph * pw % 128 == 0)
        assert limit == 0 or limit < len(slices) * ph * pw                  # a limit splits the cube into groups
    assert any(stacks) and not all(stacks)
    assert sum(any(c.form == "shuffled" for c in slices) for slices, _ in cubes) >= 2
    assert sum(limit > 0 for _, limit in cubes) >= 2
    assert len({c.kind for slices, _ in cubes for c in slices}) == len(mc.KINDS)
