"""The generators of tests/seed_cases.py reach what they claim: proven here on numpy and the CPU oracle, so that
tests/test_gpu_seed_regimes.py does not only believe it.  No GPU."""
import numpy as np
import pytest

import oracle_lib as ol
import seed_cases as sc

S = sc.segment_cases()
M = sc.minima_cases()


def _shape(case):
    return case[1].shape


def test_every_family_is_there_and_names_are_unique():
    assert {c[3]["family"] for c in S} == {"S1", "S2", "S3", "S4", "S5", "S6", "S7"}
    assert {c[2]["family"] for c in M} == {"M1", "M2", "M3", "M4", "M5"}
    assert len({c[0] for c in S}) == len(S) and len({c[0] for c in M}) == len(M)
    assert {c[0].split("/")[3] for c in S} == set(sc.KINDS)
    for name, img, seeds, facts in S:
        h, w = img.shape
        assert img.dtype == np.uint8 and seeds.dtype == np.int64 and seeds.ndim == 2
        assert (seeds >= 0).all() and (seeds[:, 0] < h).all() and (seeds[:, 1] < w).all(), name      # every list is a valid one


def test_the_claimed_form_follows_from_the_list():
    for name, img, seeds, facts in S:
        w = img.shape[1]
        assert facts["strict"] == sc.is_strict(seeds, w), name
        assert facts["form"] == ("tables" if facts["strict"] and w % 4 == 0 and len(seeds) else "painted"), name
        if facts["family"] in ("S1", "S2", "S3", "S4", "S5"):
            assert facts["strict"], name
        if facts["family"] in ("S6", "S7"):
            assert not facts["strict"], name
    # both forms are reached by sorted dense lists, and the odd shape never takes the tables
    assert any(f["form"] == "tables" and f["family"] == "S1" for _, _, _, f in S)
    assert all(f["form"] == "painted" for _, i, _, f in S if i.shape == sc.SHAPES["C"] or i.shape == sc.SHAPES["F"])
    # S7: exactly one pair of equal neighbours, the rest strictly increasing
    for name, img, seeds, facts in sc.by_family("S7"):
        d = np.diff(sc.pixels_of(seeds, img.shape[1]))
        assert (d >= 0).all() and int((d == 0).sum()) == 1 and abs(int(np.flatnonzero(d == 0)[0]) - len(d) // 2) <= 1, name


def test_every_nibble_pattern_occurs_at_every_position_of_a_mask_word():
    total = np.zeros((8, 16), dtype=np.int64)
    for name, img, seeds, facts in S:
        if facts["form"] == "tables":
            total += sc.nibbles_by_position(seeds, img.shape)
    assert (total > 0).all(), np.argwhere(total == 0)
    # ... and in the strict lists of one single shape, the one both engines and the merging tests run at
    one = np.zeros((8, 16), dtype=np.int64)
    for name, img, seeds, facts in sc.by_family("S1", "S2", shape="A"):
        one += sc.nibbles_by_position(seeds, img.shape)
    assert (one > 0).all()


def test_the_fields_own_minima_never_reach_these_patterns():
    # why the cases exist: strict maxima are never adjacent, so a nibble never holds two neighbouring seeds
    img = sc.image("noise", 132, 264, 3)
    counts = sc.nibbles_by_position(ol.find_local_minima(img).astype(np.int64), img.shape).sum(axis=0)
    assert counts[[3, 6, 7, 11, 12, 13, 14, 15]].sum() == 0 and counts[[1, 2, 4, 8]].min() > 0


def test_full_mask_words_at_both_ends_of_a_table_chunk_and_a_full_chunk_beside_an_empty_one():
    first = last = full_next_to_empty = False
    for name, img, seeds, facts in S:
        if facts["form"] != "tables":
            continue
        words = sc.per_unit(seeds, img.shape, sc.WORD)
        per_chunk = sc.TAB_CHUNK // sc.WORD
        whole = len(words) // per_chunk * per_chunk          # (chunks that lie in the plane entirely)
        first |= bool((words[0:whole:per_chunk] == sc.WORD).any())
        last |= bool((words[per_chunk - 1:whole:per_chunk] == sc.WORD).any())
        chunks = sc.per_unit(seeds, img.shape, sc.TAB_CHUNK)
        full_next_to_empty |= any((chunks[k] == sc.TAB_CHUNK and chunks[k + 1] == 0) or (chunks[k] == 0 and chunks[k + 1] == sc.TAB_CHUNK)
                                  for k in range(len(chunks) - 1))
    assert first and last and full_next_to_empty
    name, img, seeds, _ = sc.case_named("S3/D/chunk1/")
    assert list(sc.per_unit(seeds, img.shape, sc.TAB_CHUNK)[:3]) == [0, sc.TAB_CHUNK, 0]
    name, img, seeds, _ = sc.case_named("S3/D/all_but_chunk1/")
    assert list(sc.per_unit(seeds, img.shape, sc.TAB_CHUNK)[:3]) == [sc.TAB_CHUNK, 0, sc.TAB_CHUNK]


def test_paint_segments_hold_256_seeds_and_the_painted_cases_have_such():
    for key in ("C", "F"):      # the shapes that always paint
        name, img, seeds, facts = sc.case_named(f"S1/{key}/")
        assert facts["form"] == "painted" and sc.per_unit(seeds, img.shape, sc.PAINT_SEG).max() == sc.PAINT_SEG
    # S2 at 7/8: more than 64 seeds in every whole segment -- the window walk crosses windows inside a segment
    name, img, seeds, _ = sc.case_named("S2/C/seven_eighths/")
    assert sc.per_unit(seeds, img.shape, sc.PAINT_SEG)[:-1].min() > 3 * 64


def test_runs_straddle_a_table_chunk():
    for name, img, seeds, facts in sc.by_family("S4"):
        p = sc.pixels_of(seeds, img.shape[1])
        assert p[0] == sc.TAB_CHUNK - 31 and (np.diff(p) == 1).all() and p[-1] >= sc.TAB_CHUNK, name
    assert sorted({len(c[2]) for c in sc.by_family("S4", shape="D")}) == [64, 65, 256, 257, 4096, 4097]


def test_the_ends_of_the_plane():
    for name, img, seeds, facts in sc.by_family("S5"):
        npx = img.size
        p = sc.pixels_of(seeds, img.shape[1])
        if "last_word" in name:
            assert 0 < npx % 32 == len(p) and p[-1] == npx - 1 and p[0] == npx - npx % 32, name
        elif "pixel0" in name:
            assert list(p) == [0]
        else:
            assert list(p) == [npx - 1]
    assert any(f["form"] == "tables" for n, _, _, f in sc.by_family("S5") if "last_word" in n)


def test_one_list_is_longer_than_the_plane():
    name, img, seeds, facts = sc.case_named("S6/A/all_then_reversed/")
    assert len(seeds) == 2 * img.size > img.size


# ---- closed forms that do not rest on the oracle, and the oracle's agreement with them ---------------------------------------------

@pytest.mark.parametrize("key", ["A", "C", "E"])
def test_every_pixel_a_seed_closed_forms(key):
    name, img, seeds, _ = sc.case_named(f"S1/{key}/")
    h, w = img.shape
    want = (np.arange(h * w, dtype=np.uint64) + 1).reshape(h, w)
    assert (sc.painted(seeds, img.shape) == want).all()
    assert (ol.segment_arrival(img, seeds) == want).all() and (ol.segment(img, seeds) == want).all()
    twice = sc.then_reversed(seeds)
    want2 = (2 * h * w - np.arange(h * w, dtype=np.uint64)).reshape(h, w)      # pixel p: the reversed copy's entry 2 H W - 1 - p
    assert (sc.painted(twice, img.shape) == want2).all()
    assert (ol.segment_arrival(img, twice) == want2).all()


def test_the_oracle_paints_duplicates_as_the_rule_says():
    # on the seed pixels the result is the painted plane, whatever floods around them
    for name, img, seeds, facts in sc.by_family("S6", "S7"):
        got = ol.segment_arrival(img, seeds)
        paint = sc.painted(seeds, img.shape)
        assert (got[paint != 0] == paint[paint != 0]).all(), name


# ---- images whose maxima are the case ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", M, ids=[c[0] for c in M])
def test_maxima_of_the_constructed_images(case):
    name, img, facts = case
    h, w = img.shape
    got = ol.find_local_minima(img).astype(np.int64).reshape(-1, 2)
    brute = sc.strict_maxima(img)
    assert got.shape == brute.shape and (got == brute).all(), name       # the oracle against eight shifted comparisons
    if facts["want"] is not None:
        want = facts["want"]
        assert got.shape == want.shape and (got == want).all(), name      # ... and against the construction
    if facts["family"] == "M1":
        assert len(got) == ((h - 1) // 2) * ((w - 1) // 2)
    if facts["family"] == "M2":
        assert len(got) == ((h - 2) // 2) * ((w - 2) // 2)
    if facts["family"] == "M3" and facts["want"] is not None and h * w > 100:
        n = ((h - 1) // 2) * ((w - 1) // 2)
        assert 0 < len(got) < n and len(got) == n - len([k for k in range(n) if k % 3 == 2 or k % 5 == 4])
    if facts["family"] == "M4":
        assert (got[:, 0] >= 1).all() and (got[:, 0] <= h - 2).all() and (got[:, 1] >= 1).all() and (got[:, 1] <= w - 2).all()
        if h >= 9 and w >= 9:
            assert facts["border_peaks"] >= 4
            for sel in (got[:, 0] == 1, got[:, 0] == h - 2, got[:, 1] == 1, got[:, 1] == w - 2):
                assert sel.any(), name
            for edge in (img[0], img[-1], img[:, 0], img[:, -1]):
                assert (edge == facts["peak"]).any(), name
    if h >= 5 and w >= 5:
        assert len(got) > 0 and facts["peak"] in img, name


def test_bytes_254_and_255_enter_the_comparison():
    assert any(f["peak"] == 255 and f["floor"] == 254 and 255 in img and 254 in img for _, img, f in M)


def test_a_full_step_of_the_compaction_is_reached():
    # rows of 2049 pixels and more: 16 maxima in each of the 64 groups of 32 pixels a wave takes per step
    for shape in ((9, 2080), (9, 2084), (40, 2049)):
        name, img, facts = sc.minima_named(f"M1/{shape[0]}x{shape[1]}/")
        got = ol.find_local_minima(img).astype(np.int64)
        row = got[got[:, 0] == 1][:, 1]
        groups = np.bincount(row // 32, minlength=sc.MINIMA_STEP)
        assert (groups[:sc.MINIMA_STEP] == 16).all(), name
    assert {(9, 2080), (5, 4), (5, 8), (3, 3)} <= {c[1].shape for c in M}
    assert any("offset" in f and f["row_stride"] != img.shape[1] and f["offset"] % 4 == 1 for _, img, f in M)
