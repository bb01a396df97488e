"""The planted planes of tests/planted_cases.py reach what they claim, and their reference is right: proven here on the CPU,
so that tests/test_gpu_planted_stamps.py does not only believe it.  No GPU."""
import numpy as np
import pytest

import planted_cases as pc
from numpy_engine import NumpyBlockEngine

FULL_CORRIDORS = [("rows", "rows/776"), ("rows", "rows/774"), ("columns", "columns/260")]
ALL_CORRIDORS = FULL_CORRIDORS + [(n.split("/")[1], n) for n in pc.CASES if n.startswith(("high/", "twin/"))]


def _jacobi(img, t0, max_level):
    eng = NumpyBlockEngine(img, np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.int64), max_level=max_level)
    eng._k()[:] = t0
    changed = eng.relax()
    return eng._k().copy(), changed, eng.ring_overflow


def _with_facts(name):
    """(img, t0, max_level, facts) of a corridor case, in the orientation of its generator: corridors along the rows."""
    parts = name.split("/")
    if parts[0] == "high":
        img, t0, ml, facts = pc.high_rings(parts[1], int(parts[2]), with_facts=True)
    elif parts[0] == "twin":
        img, t0, ml, facts = pc.overflow_twin(parts[1], int(parts[2]), with_facts=True)
    elif parts[0] == "rows":
        img, t0, ml, facts = pc.rows(w=int(parts[1]), with_facts=True)
    else:
        img, t0, ml, facts = pc.columns(with_facts=True)
    return img, t0, ml, facts


def _pairs(name):
    img, t0, ml = pc.CASES[name]()
    return pc.fixpoint_pairs(img, t0, ml)


def test_the_case_list_is_what_the_families_promise():
    assert len([n for n in pc.CASES if n.startswith("random/")]) >= 16
    assert len(pc.TWINS) == 6 and {n.split("/")[2] for n in pc.TWINS} == {"7", "253", "254"}
    assert pc.CASES["rows/776"]()[0].shape == (131, 776) and pc.CASES["rows/774"]()[0].shape == (131, 774)
    assert pc.CASES["columns/260"]()[0].shape == (200, 260)
    assert pc.LAST_RING == (1 << 24) - 2


@pytest.mark.parametrize("name", list(pc.CASES))
def test_no_planted_stamp_is_one_the_write_back_refuses(name):
    img, t0, ml = pc.CASES[name]()
    assert img.dtype == np.uint8 and t0.dtype == np.uint32 and img.shape == t0.shape
    finite = (t0 != 0) & (t0 != pc.KEY_INF)
    assert (t0[finite] < pc.KEY_INF).all()
    ring = t0[finite] & pc.RING_MASK
    assert (ring >= 1).all() and (ring <= pc.LAST_RING).all()
    assert finite.any()


@pytest.mark.parametrize("i", range(pc.N_RANDOM))
def test_random_planes_equal_the_jacobi_engine_and_cannot_carry(i):
    img, t0, ml = pc.random_case(i)
    h, w = img.shape
    assert 33 <= h <= 70 and 250 <= w <= 530 and ml == (254 if (i // 2) % 2 == 0 else 100)
    assert set(np.unique(img)) <= set(pc.RANDOM_BYTES)
    finite = (t0 != 0) & (t0 != pc.KEY_INF)
    # ring + pixel count below 2^24 - 1: no transient stamp, on any schedule, reaches the refused ring
    assert int((t0[finite] & pc.RING_MASK).max()) + h * w < (1 << 24) - 1
    assert 0.12 < finite.mean() < 0.18 and 0.01 < (t0 == 0).mean() < 0.03
    assert finite[1:-1, 1:-1].any() and (finite[0].any() or finite[:, 0].any())      # interior and border both hold stamps
    want, overflow = pc.reference(f"random/{i:02d}")
    got, changed, flagged = _jacobi(img, t0, ml)
    assert changed and not overflow and not flagged
    assert (got == want).all()


def test_random_planes_cover_both_width_classes_levels_and_the_high_ring():
    cases = [pc.random_case(i) for i in range(pc.N_RANDOM)]
    assert {(c[0].shape[1] % 4 == 0, c[2]) for c in cases} == {(True, 254), (True, 100), (False, 254), (False, 100)}
    assert {c[0].shape for c in cases} >= {(33, 250), (70, 530)}
    for img, t0, ml in cases:
        rings = set(np.unique(t0[(t0 != 0) & (t0 != pc.KEY_INF)] & pc.RING_MASK).tolist())
        assert rings == {1, 2, 100, min(0xFFF000, (1 << 24) - 2 - img.size)}
    # the high rings survive into the fixpoint: the kernels' arithmetic is fed large numbers, not only the start plane
    assert all(int((pc.reference(f"random/{i:02d}")[0] & pc.RING_MASK).max()) > 0xFF0000 for i in range(pc.N_RANDOM))


# cut-down corridor planes: the Jacobi stand-in needs as many sweeps as a corridor is long
CUT = [("rows", dict(w=300, h=21)), ("columns", dict(w=30, h=80))]


@pytest.mark.parametrize("family,shape", CUT)
@pytest.mark.parametrize("level,max_level,top", [(7, 254, False), (7, 254, True), (253, 253, True), (254, 254, True)])
def test_cut_down_corridors_equal_the_jacobi_engine(family, shape, level, max_level, top):
    gen = pc.rows if family == "rows" else pc.columns
    img, t0, ml = gen(level=level, max_level=max_level, top=top, **shape)
    want, overflow = pc.planted_fixpoint(img, t0, ml)
    got, changed, flagged = _jacobi(img, t0, ml)
    assert changed and not overflow and not flagged
    assert (got == want).all()
    if top:
        assert int((want[want < pc.KEY_INF] & pc.RING_MASK).max()) == pc.LAST_RING
    # ... and with one source raised both refuse, the stand-in by the library's rule
    img, t0, ml = gen(level=level, max_level=max_level, top=True, raised=3, **shape)
    assert pc.planted_fixpoint(img, t0, ml)[1]
    assert _jacobi(img, t0, ml)[2]


@pytest.mark.parametrize("family,name", FULL_CORRIDORS)
def test_blockers_cover_every_lane_and_band_position_in_both_directions(family, name):
    img, t0, ml, facts = _with_facts(name)
    residues, modulus = (pc.LANE_RESIDUES, 256) if family == "rows" else (pc.BAND_RESIDUES, 64)
    assert set(pc.LANE_RESIDUES) == {4 * lane + c for lane in (0, 15, 16, 31, 32, 47, 48, 63) for c in range(4)}
    for direction in (0, 1):
        mine = [f for f in facts if f["direction"] == direction]
        assert {f["blocker_at"] % modulus for f in mine} >= set(residues), (name, direction)
        assert {f["kind"] for f in mine} == {0, 1, 2}
        assert {f["blocker"] for f in mine if f["kind"] == pc.KIND_LEVEL} == set(pc.BLOCKER_LEVELS)
        assert len({f["blocker_at"] // modulus for f in mine}) >= 3      # more than one tile along the corridor
    # every lane (band row) group meets a level blocker and a wall
    for direction in (0, 1):
        for group in {r // 4 for r in residues}:
            kinds = {f["kind"] for f in facts if f["direction"] == direction and (f["blocker_at"] % modulus) // 4 == group}
            assert len(kinds) >= 2, (name, direction, group)
    # the facts describe the plane: one-pixel corridors on every second line, sources on the two border lines only
    lines = img if family == "rows" else img.T
    start = t0 if family == "rows" else t0.T
    assert (lines[0::2] == 255).all() and (start[:, 1:-1] == pc.KEY_INF).all()
    for f in facts:
        y, x = f["line"], f["blocker_at"]
        assert lines[y, x] == f["blocker"] and (np.delete(lines[y, 1:-1], x - 1) == f["level"]).all()
        assert {sx for sx, _, _ in f["sources"]} == set(np.flatnonzero(start[y] != pc.KEY_INF).tolist())
        assert len(f["sources"]) == (2 if f["kind"] == pc.KIND_WALL_TWO_FRONTS else 1)


@pytest.mark.parametrize("family,name", ALL_CORRIDORS)
def test_every_corridor_has_the_value_the_closed_form_gives(family, name):
    img, t0, ml, facts = _with_facts(name)
    levels, rings = _pairs(name)
    if family == "columns":
        img, levels, rings = img.T, levels.T, rings.T
    assert (levels[0::2, 1:-1] == 255).all()      # the walls between the corridors
    for f in facts:
        y = f["line"]
        want = pc.corridor_closed_form(img[y].tolist(), f["level"], f["sources"], ml)
        assert list(zip(levels[y].tolist(), rings[y].tolist())) == want, (name, y)


@pytest.mark.parametrize("family,name", FULL_CORRIDORS)
def test_the_far_side_of_every_blocker(family, name):
    # spelt out for the plain families (corridor level 7, every blocker level is higher): what lies right behind the blocker
    img, t0, ml, facts = _with_facts(name)
    levels, rings = _pairs(name)
    if family == "columns":
        levels, rings = levels.T, rings.T
    length = levels.shape[1]
    for f in facts:
        y, x = f["line"], f["blocker_at"]
        (sx, step, ring) = f["sources"][0]
        at = (int(levels[y, x]), int(rings[y, x]))
        behind = (int(levels[y, x + step]), int(rings[y, x + step]))
        before = (int(levels[y, x - step]), int(rings[y, x - step]))
        assert before == (7, ring + abs(x - step - sx))
        if f["kind"] == pc.KIND_LEVEL:
            assert at == (f["blocker"], 1) and behind == (f["blocker"], 2)
            end = length - 2 if step == 1 else 1
            assert (int(levels[y, end]), int(rings[y, end])) == (f["blocker"], 1 + abs(end - x))
        elif f["kind"] == pc.KIND_WALL:
            assert at == (255, 0) and behind == (255, 0)
            assert (levels[y, x + step:length - 1] if step == 1 else levels[y, 1:x]).min() == 255
        else:
            (sx2, step2, ring2) = f["sources"][1]
            assert at == (255, 0) and behind == (7, ring2 + abs(x + step - sx2))


@pytest.mark.parametrize("family", ["rows", "columns"])
@pytest.mark.parametrize("level,max_level", pc.HIGH_LEVELS)
def test_high_rings_end_exactly_on_the_last_ring_of_the_contract(family, level, max_level):
    name = f"high/{family}/{level}"
    img, t0, ml, facts = _with_facts(name)
    assert ml == max_level
    levels, rings = _pairs(name)
    assert not pc.beyond_contract(levels, rings).any() and not pc.reference(name)[1]
    finite = levels < 255
    assert int(rings[finite].max()) == pc.LAST_RING
    assert set(levels[finite & (rings == pc.LAST_RING)].tolist()) == {level}
    # every source's flood ends on it, not only the longest corridor's
    interior = np.zeros_like(finite)
    interior[1:-1, 1:-1] = True
    assert int((interior & (rings == pc.LAST_RING)).sum()) == sum(len(f["sources"]) for f in facts)


@pytest.mark.parametrize("name", pc.TWINS)
def test_overflow_twins_need_one_ring_more_at_exactly_one_pixel(name):
    family, level = name.split("/")[1], int(name.split("/")[2])
    img, t0, ml, facts = _with_facts(name)
    base_img, base_t0, base_ml = pc.high_rings(family, level)
    assert (img == base_img).all() and ml == base_ml
    assert int((t0 != base_t0).sum()) == 1 and int((t0.astype(np.int64) - base_t0).max()) == 1      # one source, one ring
    levels, rings = _pairs(name)
    bad = pc.beyond_contract(levels, rings)
    assert pc.reference(name)[1] and int(bad.sum()) == 1
    y, x = (int(v[0]) for v in np.nonzero(bad))
    assert (int(levels[y, x]), int(rings[y, x])) == (level, pc.LAST_RING + 1)
    # the far end of the raised corridor's first run
    f = facts[pc.TWIN_CORRIDOR[family]]
    sx, step, _ = f["sources"][0]
    line, pos = (y, x) if family == "rows" else (x, y)
    assert line == f["line"] and 1 <= pos <= (img.shape[1] if family == "rows" else img.shape[0]) - 2
    far = (levels[y, x + step], rings[y, x + step]) if family == "rows" else (levels[y + step, x], rings[y + step, x])
    assert int(far[0]) != level or int(far[1]) != pc.LAST_RING + 2      # nothing behind it goes on counting
    # everything else is the high-ring plane
    base_levels, base_rings = _pairs(f"high/{family}/{level}")
    same = np.ones_like(bad)
    if family == "rows":
        same[f["line"]] = False
    else:
        same[:, f["line"]] = False
    assert (levels[same] == base_levels[same]).all() and (rings[same] == base_rings[same]).all()
