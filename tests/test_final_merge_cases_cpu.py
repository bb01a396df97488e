"""The generators of tests/final_merge_cases.py are in the regimes they claim: proven here on the CPU oracle, so that
tests/test_gpu_final_merge.py does not only believe it.  No GPU.  Every regime is asserted with a count, never as "no
counter-example"."""
import numpy as np
import pytest

import final_merge_cases as fm
import oracle_lib as ol

D = fm.d_cases()
L = fm.l_cases()

_ORACLE = {}


def oracle(case):
    """(segmenting labels, merged labels, tile_min) of a case, once."""
    name, img, seeds, facts = case
    if name not in _ORACLE:
        ps = fm.plane_seeds(case)
        seg = ol.segment_arrival(img, ps, max_level=facts["max_level"], edge=facts["edge"])
        merged = ol.merge_arrival(img, ps, max_level=facts["max_level"], edge=facts["edge"])
        _ORACLE[name] = (seg, merged, fm.classify(seg))
    return _ORACLE[name]


def test_names_shapes_kinds_and_lists():
    names = [c[0] for c in fm.all_cases()]
    assert len(set(names)) == len(names)
    for case in fm.all_cases():
        name, img, seeds, facts = case
        ph, pw = fm.plane_shape(case)
        ps = fm.plane_seeds(case)
        assert img.dtype == np.uint8 and seeds.dtype == np.int64 and seeds.ndim == 2 and seeds.shape[1] == 2, name
        assert (ps >= 0).all() and (ps[:, 0] < ph).all() and (ps[:, 1] < pw).all(), name      # every entry is in the plane
        assert (seeds >= 0).all(), name
    plain = [c for c in D if not c[3]["edge"] and c[3]["max_level"] == 254 and "two_lakes" not in c[0]]
    assert {c[1].shape for c in plain} == set(fm.D_SHAPES)
    for tag in ("then_reversed", "thrice", "first_again", "shuffled", "border_top", "corner_br"):      # every list meets every kind
        assert {c[0].split("/")[3] for c in plain if c[0].split("/")[2] == tag} == set(fm.KINDS), tag
    assert {c[3]["max_level"] for c in D} == {31, 100, 254}
    assert {(c[3]["edge"], c[3]["shift"]) for c in D} == {(False, False), (True, False), (True, True)}
    assert len({fm.plane_shape(c) for c in D if c[3]["edge"]}) == 2
    assert {c[1].shape for c in L} >= {(64, 4480), (64, 8320), (832, 320), (192, 2816)}
    assert any(1 <= c[1].shape[0] % 64 <= 3 and 1 <= c[1].shape[1] % 64 <= 3 for c in L)
    assert all(len(c[2]) <= 13 for c in L) and max(c[1].size for c in fm.all_cases()) == 192 * 2816      # (64 x 8320 is the widest)


def test_the_tile_classification_on_hand_made_planes():
    seg = np.zeros((66, 130), dtype=np.uint64)
    seg[1:-1, 1:-1] = 7
    seg[0, 0] = 1                      # a corner never counts
    seg[0, 5] = 3                      # a border pixel does
    seg[40, 100] = 0                   # one interior pixel uncoloured: tile (0, 1) is general
    seg[65, 129] = 2
    assert fm.classify(seg).tolist() == [[3, 0, 7], [7, 7, 7]]
    # tiles that hold border pixels only (row 64 of 65, column 128 of 129) have no interior pixel: never one lake
    assert fm.classify(np.full((65, 129), 7, dtype=np.uint64)).tolist() == [[7, 7, 0], [0, 0, 0]]
    r = fm.runs(np.array([[5, 0, 4, 4, 4]] * 27, dtype=np.uint64))      # 135 tiles, 5 per row: 64 = (12, 4), 128 = (25, 3)
    assert len(r) == 54 and r[0]["lane0"] == 0 and r[1]["lane0"] == 2 and r[1]["mins"].tolist() == [4, 4, 4]
    assert [x["t0"] for x in r if x["crosses"]] == [62, 127] and r[25]["crosses"] == [64] and r[51]["crosses"] == [128]


# ---- family D ---------------------------------------------------------------------------------------------------------------------------

def _lake_of_tile(case, tile):
    """The oracle's id of the lake the tile's interior pixels belong to (one-lake tile: there is one)."""
    seg, merged, _ = oracle(case)
    inner = fm.interior_mask(seg.shape)
    sl = (slice(tile[0] * fm.UT, (tile[0] + 1) * fm.UT), slice(tile[1] * fm.UT, (tile[1] + 1) * fm.UT))
    ids = np.unique(merged[sl][inner[sl]])
    assert len(ids) == 1 and ids[0] != 0, (case[0], tile, ids)
    return int(ids[0])


def test_undercut_cases_hold_an_overwritten_colour_below_the_lake_id_in_a_one_lake_tile():
    proven = {"one": 0, "general": 0}
    by_name = {c[0]: c for c in D}
    for case in D:
        name, img, seeds, facts = case
        if not facts["undercut"]:
            continue
        seg, merged, tile_min = oracle(case)
        ps = fm.plane_seeds(case)
        assert facts["entries"], name
        for i in facts["entries"]:
            r, c = (int(v) for v in ps[i])
            assert not fm.is_corner(r, c, seg.shape), name
            assert seg[r, c] != i + 1 and seg[r, c] > i + 1, (name, i)                  # painted with another, later colour
            assert not (seg == i + 1).any(), (name, i)                                  # ... and found nowhere in the plane
            t = fm.tile_of(r, c)
            if facts["twin"] == "one":
                assert tile_min[t] != 0, (name, i, t)
                assert i + 1 < _lake_of_tile(case, t) <= tile_min[t], (name, i)
                assert merged[r, c] == _lake_of_tile(case, t)
            else:
                assert tile_min[t] == 0, (name, i, t)
                one = by_name[name.rsplit("/", 1)[0] + "/one"]
                assert (one[2] == seeds).all() and int((one[1] != img).sum()) == len({fm.tile_of(*ps[j]) for j in facts["entries"]}), name
                assert 0 < merged[r, c] and i + 1 < merged[r, c], (name, i)             # the same id rule on the general path
        proven[facts["twin"]] += 1
    assert proven["one"] >= 50 and proven["general"] >= 45, proven
    # ... on every shape, kind and option the family has
    flagged = [c for c in D if c[3]["undercut"]]
    assert {c[1].shape for c in flagged} >= set(fm.D_SHAPES) | {(64, 192)}
    assert {(c[3]["edge"], c[3]["shift"]) for c in flagged} == {(False, False), (True, False), (True, True)}
    assert {c[3]["max_level"] for c in flagged} == {31, 100, 254}
    assert sum(len(c[3]["entries"]) == 2 for c in flagged) >= 6
    # undercut entries in thin tiles (fewer than 64 rows or columns) as well as in whole ones
    thin = sum(1 for c in flagged if c[3]["twin"] == "one" for i in c[3]["entries"]
               if min(fm.plane_shape(c)[0] - fm.tile_of(*fm.plane_seeds(c)[i])[0] * 64, fm.plane_shape(c)[1] - fm.tile_of(*fm.plane_seeds(c)[i])[1] * 64) < 64)
    assert thin >= 10, thin


def test_the_smallest_input_is_the_one_the_issue_names():
    name, img, seeds, facts = fm.named("D/3x3/centre_twice/")
    assert img.shape == (3, 3) and seeds.tolist() == [[1, 1], [1, 1]]
    seg, merged, tile_min = oracle((name, img, seeds, facts))
    assert merged[1, 1] == 2 and tile_min.tolist() == [[2]] and not (merged == 1).any()


def test_corner_and_border_cases_are_what_their_names_say():
    count = {"corner": 0, "border": 0}
    for case in D:
        name, img, seeds, facts = case
        tag = name.split("/")[3] if name.split("/")[1].startswith(("edge", "level")) else name.split("/")[2]
        assert (facts["where"] == "corner") == tag.startswith("corner_") and (facts["where"] == "border") == tag.startswith("border_"), name
        if facts["where"] == "interior":
            continue
        seg, merged, tile_min = oracle(case)
        ph, pw = seg.shape
        ps = fm.plane_seeds(case)
        for i in facts["entries"]:
            r, c = (int(v) for v in ps[i])
            on_border = r in (0, ph - 1) or c in (0, pw - 1)
            assert on_border and fm.is_corner(r, c, seg.shape) == (facts["where"] == "corner"), name
            want = {"corner_tl": (0, 0), "corner_tr": (0, pw - 1), "corner_bl": (ph - 1, 0), "corner_br": (ph - 1, pw - 1)}.get(tag)
            if want:
                assert (r, c) == want, name
            if tag.startswith("border_"):
                assert {"top": r == 0, "bottom": r == ph - 1, "left": c == 0, "right": c == pw - 1}[tag.split("_")[1]], name
            assert seg[r, c] > i + 1 and not (seg == i + 1).any(), name                 # overwritten
            if facts["where"] == "corner":
                assert facts["undercut"] is False and merged[r, c] == seg[r, c], name   # a corner joins nothing: it keeps its colour
        count[facts["where"]] += 1
    assert count["corner"] >= 40 and count["border"] >= 40, count
    assert {c[0].split("/")[2] for c in D if c[3]["where"] == "corner" and c[0].split("/")[1] == "66x66"} == {"corner_tl", "corner_tr", "corner_bl", "corner_br"}


def test_two_lakes_of_one_lake_tiles_each_with_an_overwritten_colour_below_its_id():
    got = [c for c in D if "two_lakes" in c[0] and c[3]["twin"] == "one"]
    assert len(got) == 3
    for case in got:
        seg, merged, tile_min = oracle(case)
        assert tile_min[0, 0] != 0 and tile_min[0, 1] == 0 and tile_min[0, 2] != 0
        a, b = _lake_of_tile(case, (0, 0)), _lake_of_tile(case, (0, 2))
        assert (a, b) == (3, 4) and (merged[:, 64:128] == 0).all()
        ps = fm.plane_seeds(case)
        assert fm.tile_of(*ps[0]) == (0, 0) and fm.tile_of(*ps[1]) == (0, 2)


def test_partial_levels_leave_general_tiles_and_the_cases_without_a_claim_make_none():
    general = no_interior = 0
    for case in D:
        if case[3]["undercut"] is None and case[3]["max_level"] != 254:
            general += int((oracle(case)[2] == 0).any())
        elif case[3]["undercut"] is None:      # a border entry whose tile has no interior pixel (row 64 of 65, column 128 of 129)
            assert case[3]["where"] == "border"
            r, c = fm.plane_seeds(case)[case[3]["entries"][0]]
            assert oracle(case)[2][fm.tile_of(r, c)] == 0
            no_interior += 1
    assert general >= 10 and no_interior >= 2, (general, no_interior)


@pytest.mark.parametrize("prefix", ["S6/A/all_then_reversed/", "S6/A/half_then_reversed/", "S6/C/all_then_reversed/", "S6/C/half_then_reversed/"])
def test_the_dense_reversed_lists_of_seed_cases_undercut_too(prefix):
    """The four S6 cases that tests/test_gpu_seed_regimes.py merges: colour 2 is overwritten, sits in a one-lake tile and lies
    below a lake id in the thousands."""
    import seed_cases as sc
    name, img, seeds, _ = sc.case_named(prefix)
    seg = ol.segment_arrival(img, seeds)
    merged = ol.merge_arrival(img, seeds)
    tile_min = fm.classify(seg)
    r, c = (int(v) for v in seeds[1])
    assert not fm.is_corner(r, c, img.shape) and seg[r, c] > 2 and not (seg == 2).any(), name
    assert tile_min[fm.tile_of(r, c)] != 0 and merged[r, c] >= 1000, (name, int(merged[r, c]))


# ---- family L ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", L, ids=[c[0] for c in L])
def test_tile_classes_follow_the_pattern(case):
    name, img, seeds, facts = case
    seg, merged, tile_min = oracle(case)
    rows = facts["pattern"]
    want = np.array([[ch == "O" for ch in r] for r in rows])
    assert want.shape == tile_min.shape and ((tile_min != 0) == want).all(), name      # every open tile floods, no other tile is one lake
    assert want.any() and not want.all()
    # sparse seeds: colours span tiles (a missed link would show)
    assert len(seeds) < int(want.sum()) and len(np.unique(seg[seg != 0])) == len(seeds)


def test_long_run_regimes_occur():
    heads = set()
    cross_single = cross_multi = 0
    where_min = {"first": 0, "interior": 0, "last": 0, "beyond": 0}
    upper_starts = {"left": 0, "at": 0, "right": 0}
    rows_ending_off_63 = 0
    lakes = []
    over_a_wave = 0
    for case in L:
        seg, merged, tile_min = oracle(case)
        ty, tx = tile_min.shape
        over_a_wave += ty * tx > fm.WAVE
        rs = fm.runs(tile_min)
        lakes.append(len(np.unique(merged[merged != 0])))
        rows_ending_off_63 += sum(1 for y in range(ty) if ty > 1 and ((y + 1) * tx - 1) % fm.WAVE != 63)
        for r in rs:
            heads.add(r["lane0"])
            if r["crosses"]:
                cross_single += ty == 1
                cross_multi += ty > 1
            mins = r["mins"]
            if len(mins) >= 3 and len(np.unique(mins)) >= 2:
                k = int(np.argmin(mins))      # the first tile that holds the run's smallest colour
                where_min["first"] += k == 0
                where_min["interior"] += 0 < k < len(mins) - 1
                where_min["last"] += k == len(mins) - 1
                where_min["beyond"] += bool(r["crosses"]) and r["t0"] + k >= r["crosses"][0]
        for u in rs:
            for lo in rs:
                if lo["ty"] == u["ty"] + 1 and u["x0"] <= lo["x1"] and lo["x0"] <= u["x1"]:      # they share a column
                    upper_starts["left" if u["x0"] < lo["x0"] else "at" if u["x0"] == lo["x0"] else "right"] += 1
    assert {0, 1, 62, 63} <= heads, sorted(heads)
    assert cross_single >= 2 and cross_multi >= 2, (cross_single, cross_multi)
    assert min(where_min.values()) >= 1, where_min
    assert min(upper_starts.values()) >= 2, upper_starts
    assert rows_ending_off_63 >= 10
    assert max(lakes) >= 3 and sum(n >= 3 for n in lakes) >= 2, lakes
    assert over_a_wave >= 4
