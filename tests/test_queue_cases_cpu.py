"""The seeded corridors of tests/queue_cases.py reach what they claim, and the oracle gives them the closed form's stamps: proven
here on the CPU, so that tests/test_gpu_queue_corridors.py does not only believe it.  No GPU."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
import planted_cases as pc
import queue_cases as qc

NEVER = np.uint64(0xFFFFFFFFFFFFFFFF)


def _with_facts(name):
    """(img, seeds, max_level, facts) of a corridor case."""
    return qc.columns(with_facts=True) if name.startswith("columns/") else qc.rows(with_facts=True, **qc.ROWS_FORMS[name])


@functools.lru_cache(maxsize=None)
def _oracle_pairs(name):
    """The oracle's stamps as two int64 planes (level, ring); never coloured: (255, 0)."""
    img, seeds, ml = qc.scalar_twin() if name == qc.SCALAR_TWIN else qc.CASES[name]()
    _, keys = ol.segment_arrival(img, seeds, max_level=ml, want_keys=True)
    never = keys == NEVER
    levels = np.where(never, 255, keys >> np.uint64(32)).astype(np.int64)
    rings = np.where(never, 0, keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return levels, rings


def test_the_case_list_is_what_the_families_promise():
    assert set(qc.CASES) == {"rows/1416", "columns/516", "serpentine/520", "rows/level253", "rows/level254", "rows/max20"}
    assert qc.CASES["rows/1416"]()[0].shape == (193, 1416) and qc.CASES["columns/516"]()[0].shape == (650, 516)
    assert qc.CASES["serpentine/520"]()[0].shape == (151, 520) and qc.scalar_twin()[0].shape == (193, 1414)
    assert [(qc.CASES[f"rows/level{lv}"]()[2], int(qc.CASES[f"rows/level{lv}"]()[0][1, 1])) for lv in (253, 254)] == [(253, 253), (254, 254)]
    assert qc.CASES["rows/max20"]()[2] == 20 and (qc.CASES["rows/max20"]()[0] == qc.CASES["rows/1416"]()[0]).all()
    assert qc.LANE_RESIDUES == tuple(4 * lane + c for lane in (0, 15, 16, 31) for c in range(4))
    for name, case in list(qc.CASES.items()) + [(qc.SCALAR_TWIN, qc.scalar_twin)]:
        img, seeds, ml = case()
        h, w = img.shape
        assert (w % 4 == 0) == (name != qc.SCALAR_TWIN)      # relax_plan offers the queue to no other width
        assert h * w < 500_000                               # every GPU test stays a matter of seconds
        assert qc.QT < h and w % qc.QT in (2, 4, 6, 8)       # more than one tile row, a last tile column of one or two patches
    assert qc.COLUMNS_SHAPE[0] % qc.QT == 4                  # ... of one patch column


@pytest.mark.parametrize("name", list(qc.CASES) + [qc.SCALAR_TWIN])
def test_seed_lists_are_strictly_increasing_and_interior(name):
    img, seeds, ml = qc.scalar_twin() if name == qc.SCALAR_TWIN else qc.CASES[name]()
    h, w = img.shape
    assert seeds.dtype == np.uint64 and seeds.ndim == 2 and seeds.shape[1] == 2 and len(seeds) >= 1
    index = seeds[:, 0].astype(np.int64) * w + seeds[:, 1].astype(np.int64)
    assert (np.diff(index) > 0).all()                        # the seed-table form
    assert (seeds[:, 0] >= 1).all() and (seeds[:, 0] <= h - 2).all() and (seeds[:, 1] >= 1).all() and (seeds[:, 1] <= w - 2).all()
    assert (img[seeds[:, 0].astype(np.int64), seeds[:, 1].astype(np.int64)] <= ml).all()


def test_seed_counts_lie_on_the_side_of_the_auto_rule_that_the_gpu_tests_rely_on():
    # run_fused_form, persistent_pass 3: 1 .. relax_tiles / 2 seeds -> the queue in flood order; up to 32 a tile -> the early schedule
    assert qc.relax_tiles(193, 1416) == 65 and qc.relax_tiles(650, 516) == 88 and qc.relax_tiles(151, 520) == 24
    for name in qc.CORRIDORS:
        img, seeds, _ = qc.CASES[name]()
        tiles = qc.relax_tiles(*img.shape)
        assert tiles // 2 < len(seeds) <= tiles * 32, name
    img, seeds, _ = qc.CASES["serpentine/520"]()
    assert 1 == len(seeds) <= qc.relax_tiles(*img.shape) // 2
    for slices, slice_h in qc.STACKS:
        cube, lists, _ = qc.stack(slices, slice_h)
        tiles = qc.relax_tiles(slices * slice_h, cube.shape[2])
        assert tiles // 2 < sum(len(s) for s in lists) <= tiles * 32


@pytest.mark.parametrize("name", ["rows/1416", "columns/516", qc.SCALAR_TWIN])
def test_blockers_cover_every_hand_over_position_in_both_directions(name):
    img, seeds, ml, facts = _with_facts(name)
    rows = not name.startswith("columns/")
    residues, lead = (qc.LANE_RESIDUES, qc.ROWS_LEAD) if rows else (qc.BAND_RESIDUES, qc.COLUMNS_LEAD)
    lines = img if rows else img.T
    length = lines.shape[1]
    assert len(facts) == (lines.shape[0] - 1) // 2
    for direction in (0, 1):
        mine = [f for f in facts if f["direction"] == direction]
        if rows:      # every kind at every residue
            for kind in (pc.KIND_LEVEL, pc.KIND_WALL, pc.KIND_WALL_TWO_FRONTS):
                assert {f["blocker_at"] % qc.QT for f in mine if f["kind"] == kind} == set(residues), (name, direction, kind)
        else:         # every residue -- the tile's first and last rows among them --, every kind in every band
            assert {f["blocker_at"] % qc.QT for f in mine} == set(range(qc.QT)), (name, direction)
            for band in range(qc.QT // 4):
                assert {f["kind"] for f in mine if f["blocker_at"] % qc.QT // 4 == band} == {0, 1, 2}, (name, direction, band)
        assert {f["blocker"] for f in mine if f["kind"] == pc.KIND_LEVEL} == set(pc.BLOCKER_LEVELS)
        assert len({f["blocker_at"] // qc.QT for f in mine}) >= 2      # more than one tile along the corridor
        # every lane (band) group meets every blocker level
        for group in {r // 4 for r in residues}:
            levels = {f["blocker"] for f in mine if f["kind"] == pc.KIND_LEVEL and f["blocker_at"] % qc.QT // 4 == group}
            assert levels == set(pc.BLOCKER_LEVELS) if rows else len(levels) >= 1, (name, direction, group)
    # the lead: every blocker lies that far from the seed that feeds it, and inside the plane
    for f in facts:
        sx, step, ring = f["sources"][0]
        assert ring == 0 and sx == (1 if f["direction"] == 0 else length - 2) and step == (1 if f["direction"] == 0 else -1)
        assert abs(f["blocker_at"] - sx) >= lead and 2 <= f["blocker_at"] <= length - 3
        assert len(f["sources"]) == (2 if f["kind"] == pc.KIND_WALL_TWO_FRONTS else 1)
        if len(f["sources"]) == 2:
            assert f["sources"][1] == (length - 1 - sx, -step, 0)
    # the facts describe the plane: one-pixel corridors on every second line, a seed exactly on every source
    assert (lines[0::2] == 255).all() and (lines[:, 0] == 255).all() and (lines[:, -1] == 255).all()
    want = sorted((f["line"], sx) if rows else (sx, f["line"]) for f in facts for sx, _, _ in f["sources"])
    assert [tuple(int(v) for v in s) for s in seeds] == want
    for f in facts:
        y, x = f["line"], f["blocker_at"]
        assert lines[y, x] == f["blocker"] and (np.delete(lines[y, 1:-1], x - 1) == f["level"]).all()
    # both tile rows (tile columns of the transpose) hold corridors of both directions and of every kind
    for half in (0, 1):
        there = [f for f in facts if f["line"] // qc.QT == half]
        assert {(f["direction"], f["kind"]) for f in there} == {(d, k) for d in (0, 1) for k in (0, 1, 2)}, (name, half)


@pytest.mark.parametrize("name", list(qc.CORRIDORS) + [qc.SCALAR_TWIN])
def test_the_oracle_gives_every_corridor_the_closed_form(name):
    img, seeds, ml, facts = _with_facts(name)
    levels, rings = _oracle_pairs(name)
    if name.startswith("columns/"):
        img, levels, rings = img.T, levels.T, rings.T
    assert (levels[0::2] == 255).all() and (levels[:, 0] == 255).all() and (levels[:, -1] == 255).all()      # walls and border
    for f in facts:
        y = f["line"]
        want = pc.corridor_closed_form(img[y].tolist(), 0, f["sources"], ml)
        assert list(zip(levels[y].tolist(), rings[y].tolist())) == want, (name, y)
    assert int(rings.max()) < 1 << 12      # no ring comes near 2^24: the carry guard is planted_cases' business


@pytest.mark.parametrize("name", ["rows/1416", "rows/max20", "rows/level253", "rows/level254"])
def test_the_far_side_of_every_blocker(name):
    # spelt out: what lies on the blocker and right behind it, per level pair
    img, seeds, ml, facts = _with_facts(name)
    levels, rings = _oracle_pairs(name)
    level = int(img[1, 1])
    floods = 0
    for f in facts:
        y, x = f["line"], f["blocker_at"]
        sx, step, _ = f["sources"][0]
        at = (int(levels[y, x]), int(rings[y, x]))
        behind = (int(levels[y, x + step]), int(rings[y, x + step]))
        assert (int(levels[y, x - step]), int(rings[y, x - step])) == (level, abs(x - step - sx))
        if f["kind"] == pc.KIND_LEVEL and f["blocker"] > ml:          # max_level 20 or 253: a level that never opens is a wall
            assert at == (255, 0) and behind == (255, 0)
        elif f["kind"] == pc.KIND_LEVEL and f["blocker"] > level:     # the flood goes on at the blocker's level
            assert at == (f["blocker"], 1) and behind == (f["blocker"], 2)
            floods += 1
        elif f["kind"] == pc.KIND_LEVEL:                              # a lower byte in a high corridor: no blocker at all
            assert at == (level, abs(x - sx)) and behind == (level, abs(x - sx) + 1)
        elif f["kind"] == pc.KIND_WALL:
            assert at == (255, 0) and behind == (255, 0)
        else:
            d = abs(x + step - f["sources"][1][0])                    # the second front, counted from the far seed
            assert at == (255, 0) and behind == ((level, d) if d else (0, 0))
    assert (floods > 0) == (level == 7)
    if name == "rows/max20":
        assert sorted(set(levels[levels < 255].tolist())) == [0, 7, 9]


def test_the_serpentine_is_one_path_with_rising_blockers_and_the_oracle_walks_it():
    img, seeds, ml, path, blockers = qc.serpentine(with_facts=True)
    h, w = img.shape
    assert ml == qc.SERPENTINE_MAX_LEVEL and [tuple(int(v) for v in s) for s in seeds] == [path[0]] == [(1, 1)]
    # a single path: consecutive pixels are 4-neighbours, no pixel twice, nothing else is open
    steps = np.abs(np.diff(np.array(path), axis=0)).sum(axis=1)
    assert (steps == 1).all() and len(set(path)) == len(path) == int((img < 255).sum())
    assert len(path) == 75 * 518 + 74 and path[-1][0] == h - 2
    assert {y // qc.QT for y, _ in path} == {0, 1}
    hops = qc.tile_hops(path)
    assert 250 < hops < 400, hops      # a chain long enough to matter, an order of magnitude inside the kernel's time budget
    # the blockers: one level higher each along the path, every residue in both directions, both tile rows
    order = [path.index((2 * b["leg"] + 1, b["blocker_at"])) for b in blockers]
    assert order == sorted(order)
    assert [b["blocker"] for b in blockers] == list(range(8, 8 + 2 * len(qc.LANE_RESIDUES))) and blockers[-1]["blocker"] < ml
    for direction in (0, 1):
        mine = [b for b in blockers if b["direction"] == direction]
        assert all(b["leg"] % 2 == direction for b in mine)
        assert sorted(b["blocker_at"] % qc.QT for b in mine) == sorted(qc.LANE_RESIDUES)
        assert {(2 * b["leg"] + 1) // qc.QT for b in mine} == {0, 1}
        assert len({b["blocker_at"] // qc.QT for b in mine}) >= 3
    # the oracle's stamps along the path are the closed form of one corridor
    levels, rings = _oracle_pairs("serpentine/520")
    ys, xs = (np.array(v) for v in zip(*path))
    line = [255] + img[ys, xs].tolist() + [255]
    want = pc.corridor_closed_form(line, 0, [(1, 1, 0)], ml)[1:-1]
    assert list(zip(levels[ys, xs].tolist(), rings[ys, xs].tolist())) == want
    assert want[-1][0] == blockers[-1]["blocker"]      # the flood reaches the path's end
    off = np.ones((h, w), dtype=bool)
    off[ys, xs] = False
    assert (levels[off] == 255).all()
    assert int(rings.max()) < 1 << 12
    # flood-order buckets of two levels (pq_shift_of: 31 <= max_level < 62): the path climbs through 17 of them
    assert len({lv >> 1 for lv, _ in want[1:]}) == 17


@pytest.mark.parametrize("slices,slice_h", qc.STACKS)
def test_stacks_put_slice_walls_inside_a_queue_tile(slices, slice_h):
    cube, lists, ml = qc.stack(slices, slice_h)
    assert cube.shape == (slices, slice_h, qc.ROWS_SHAPE[0]) and len(lists) == slices and ml == 254
    walls = [s * slice_h for s in range(1, slices)]
    assert all(y % qc.QT not in (0, qc.QT - 1) for y in walls) and slices * slice_h > qc.QT
    assert len({cube[s].tobytes() for s in range(slices)}) == slices      # no two slices alike
    for s in range(slices):
        img, seeds, _ = qc.rows(h=slice_h, shift=5 * s)
        assert (cube[s] == img).all() and (lists[s] == seeds).all()
        index = seeds[:, 0].astype(np.int64) * img.shape[1] + seeds[:, 1].astype(np.int64)
        assert (np.diff(index) > 0).all()
