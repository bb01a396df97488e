"""The cut catalogue on the CPU: on every case the GPU tests use, the reference of tests/tree_cut_catalogue_ref.py agrees with the
same fold over the planes derived without a tree walk, with the hierarchy's catalogue where the two definitions coincide, and
with the record of the whole plane when a cut's regions and its hidden pixels are joined; and the cases reach the regimes they
are there for (conditions on the oracle's planes, not measurements)."""
import numpy as np
import pytest

import lake_stats_ref as ls
import tree_cut_catalogue_ref as cc
import tree_cut_stats_ref as ts


def _cases():
    return [(name,) + cc.cuts_of(name) for name in cc.ALL] + [("random48x52/32", cc.field("random48x52"), cc.THIRTY_TWO)]


@pytest.mark.parametrize("name", cc.ALL)
def test_the_fold_over_the_walk_equals_the_fold_over_the_planes(name):
    f, cuts = cc.cuts_of(name)
    v = cc.weights_of(f)
    for cut in cuts:
        other = ls.records_by_label(f.cut_planes(cut), v, f.n_seeds + 1)
        assert ls.mismatch(cc.fold(f, cut), other) is None, (name, cut)


@pytest.mark.parametrize("name", cc.ALL)
def test_a_history_plane_shows_the_lakes_that_die_next_as_the_catalogue_measured_them(name):
    """Cut() with show_level = merge_level = L: a node that dies at L + 1 is shown as M_c, the lake when it died -- the one
    case in which a region's record is the hierarchy's (lake_stats_ref.expected's: the field's own catalogue)."""
    f = cc.field(name)
    _, want = ls.expected(f.img, f.seeds, f.weights, f.max_level, f.edge, f.seed_shift)
    assert ls.mismatch(want, f.stats) is None
    deaths = np.unique(f.death[(f.death != ts.ALIVE) & (f.death >= 1) & f.ex])
    picks = sorted({int(deaths[0]), int(deaths[len(deaths) // 2]), int(deaths[-1])}) if deaths.size else []      # (`adjacent`: its one death is at level 0)
    for d in picks:
        rec = cc.fold(f, cc.Cut(show_level=d - 1, merge_level=d - 1))
        nodes = np.flatnonzero((f.death == d) & f.ex)
        assert nodes.size and ls.mismatch(rec[nodes], f.stats[nodes]) is None, (name, d)
    rec = cc.fold(f, cc.Cut(show_level=f.max_level, merge_level=f.max_level))
    alive = np.flatnonzero((f.death == ts.ALIVE) & f.ex)
    alive = alive[alive != 0]
    assert alive.size and ls.mismatch(rec[alive], f.stats[alive]) is None, name


@pytest.mark.parametrize("name", cc.ALL)
def test_hidden_record_of_a_cut_that_shows_every_level_is_catalogue_record_0(name):
    f = cc.field(name)
    *_, hid = cc.expected(f, [cc.Cut(show_level=254)])
    assert ls.mismatch(hid[:1], f.stats[:1]) is None, name


def test_regions_and_hidden_pixels_join_to_the_whole_plane():
    for name, f, cuts in _cases():
        whole = cc.whole_plane(f)
        lakes, region, offsets, hidden, hid = cc.expected(f, cuts)
        for k in range(len(cuts)):
            lo, hi = int(offsets[k]), int(offsets[k + 1])
            got = ls.join(np.concatenate([region[lo:hi], hid[k: k + 1]]))
            assert ls.mismatch(np.array([got]), np.array([whole])) is None, (name, cuts[k])
            assert int(lakes[lo:hi, 1].sum()) + int(hidden[k]) == f.seg.size


def test_no_region_record_is_the_catalogue_record_in_general():
    """Why the hierarchy's catalogue cannot stand in: under a pruning cut most regions differ from M_c of their colour."""
    f, cuts = cc.cuts_of("random48x52")
    lakes, region, offsets, _, _ = cc.expected(f, [cc.Cut(min_area=4)])
    differ = sum(ls.mismatch(region[i: i + 1], f.stats[int(lakes[i, 0]): int(lakes[i, 0]) + 1]) is not None for i in range(len(lakes)))
    assert differ >= len(lakes) // 4, (differ, len(lakes))


# ---- the regimes -------------------------------------------------------------------------------------------------------------------

def test_a_run_shows_more_regions_than_half_a_table():
    """More than 256 distinct regions in one run of 1024 pixels: the table is written out in mid-run, and probes overflow."""
    f, cuts = cc.cuts_of("checker48x52")
    most = max(cc.regions_per_run(f.cut(cuts[0])))
    assert most > 256, most
    assert int(cc.expected(f, cuts[:1])[2][1]) > 1024      # more regions a cut than two tables hold
    g, _ = cc.cuts_of("all_seeds48x52")      # every pixel a seed: seeds that touch die at level 0, so that field tests the chains, not the table
    assert g.n_seeds == 48 * 52 and (g.death == 0).sum() > 2000


def test_regions_span_runs_and_peaks_tie_across_runs():
    spans = ties = False
    for name, f, cuts in _cases():
        v = cc.weights_of(f).ravel()
        for cut in cuts:
            flat = f.cut(cut).ravel()
            run = np.arange(flat.size) // cc.RUN
            rec = cc.fold(f, cut)
            for a in np.unique(flat[flat != 0])[:64]:
                px = np.flatnonzero(flat == a)
                spans |= np.unique(run[px]).size >= 2
                top = px[v[px] == rec["w_max"][a]]
                ties |= top.size >= 2 and np.unique(run[top]).size >= 2
            if spans and ties:
                return
    assert spans and ties, (spans, ties)


def test_constant_weights_put_every_peak_on_the_first_pixel():
    f, cuts = cc.cuts_of("random48x52_const")
    for cut in cuts:
        plane, rec = f.cut(cut).ravel(), cc.fold(f, cut)
        for a in np.unique(plane):
            assert rec["peak_pixel"][a] == np.flatnonzero(plane == a)[0] and rec["w_min"][a] == rec["w_max"][a] == 7


def test_a_weighted_row_sum_passes_two_to_the_32():
    f, cuts = cc.cuts_of("staircase_u16max")
    assert f.shape == (257, 260)
    _, region, _, _, hid = cc.expected(f, cuts)
    assert max(int(region["sum_wr"].max()), int(hid["sum_wr"].max())) >= 1 << 32


def test_a_cut_and_its_repeat_travel_together():
    _, cuts = cc.cuts_of("random48x52")
    keys = [c.key() for c in cuts]
    assert len(set(keys)) < len(keys)
    for at, of in cc.REPEATS_32:
        assert at != of and cc.THIRTY_TWO[at].key() == cc.THIRTY_TWO[of].key()
    assert len(cc.THIRTY_TWO) == 32


def test_some_cut_hides_pixels_of_coloured_basins():
    hit = False
    for name, f, cuts in _cases():
        for cut in cuts:
            if cut.show_level < 254:
                hit |= bool(((f.cut(cut) == 0) & (f.seg != 0)).any())
    assert hit
