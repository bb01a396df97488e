"""The reference's proof that the inputs of tests/extreme_cases.py are what they claim, without a GPU: the one-run derivation of
every product equals the literal definitions (merge_tree_ref, lake_stats_ref, the sweep oracle's hook), a stitched chain equals
the oracle on the whole plane for every product the GPU tests compare, and the planes reach the regimes they are meant for."""
import numpy as np
import pytest

import extreme_cases as xc
import lake_stats_ref as ls
import merge_tree_ref as mt
import merging_cases as mc
import oracle_lib as ol


@pytest.mark.parametrize("kind,h,w,edge,max_level", [("noise", 60, 70, False, 254), ("few", 40, 50, True, 17), ("walls", 30, 33, False, 254)])
def test_products_equal_the_literal_definitions(kind, h, w, edge, max_level):
    """Duplicate seeds included (the `repeats` form): colours that never existed, deaths at level 0."""
    rng = np.random.default_rng(h)
    img = mc.make_field(kind, h, w, rng, 3 if kind == "few" else 40)
    seeds = mc.make_seeds("repeats", h, w, h * w // 12, rng)
    levels = [0, max_level // 2, max_level]
    e = mc.expected(mc.Case(f"extreme-{kind}", img, seeds, kind, "repeats", max_level, edge, False, levels))
    wt = xc.weights_u16(img.shape, 3)
    p = xc.products(img, seeds, max_level, edge, levels=levels, weights=wt)
    assert (p.tree == e.tree).all() and (p.labels == e.labels).all()
    assert (p.final == ol.merge_arrival(img, seeds, max_level=max_level, edge=edge)).all()
    _, keys = ol.segment_arrival(img, seeds, max_level=max_level, edge=edge, want_keys=True)
    assert xc.stamps_mismatch(xc.pack_stamps(keys), p.stamps) is None
    for L in levels:
        assert (p.planes[L] == e.planes[L]).all() and (p.seg_planes[L] == e.seg_planes[L]).all()
    seg = {}
    ol.segment(img, seeds, max_level=max_level, edge=edge, hook=lambda l, m, i, c: seg.__setitem__(int(l), ol.find_lake_sizes(c)))
    for L in range(max_level + 1):
        for got, want in zip(p.lakes[L], e.lakes[L]):
            assert np.array_equal(np.asarray(got), np.asarray(want)), L
        cols, areas, unc = p.seg_lakes[L]
        assert unc == seg[L][0] and np.array_equal(np.flatnonzero(seg[L][1:]) + 1, cols) and np.array_equal(seg[L][cols], areas), L
    planes, ps = mt.oracle_planes(img, seeds, max_level, edge, False)
    want = ls.stats_from_planes(planes, ps, ls.plane_weights(img, wt, edge), e.death, e.ex)
    assert ls.mismatch(p.stats, want) is None, ls.mismatch(p.stats, want)


CHAIN_LINES = 20 * xc.P + 57


@pytest.mark.parametrize("shape", [(CHAIN_LINES, 3), (CHAIN_LINES, 4), (CHAIN_LINES, 8), (3, CHAIN_LINES), (4, CHAIN_LINES), (8, CHAIN_LINES)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_stitched_chain_equals_the_oracle_on_the_whole_plane(shape):
    """20 pieces and a remainder of 57 lines: labels, stamps, final labels, history planes, tree records and the catalogue (the
    per-level lake lists are not asked for on chains: tests/test_gpu_extreme_shapes.py)."""
    ch = xc.Chain(shape)
    assert ch.n_full == 20 and ch.rem == 57 and len(set(ch.which.tolist())) == 4
    assert np.array_equal(ch.seeds, ol.find_local_minima(ch.img).astype(np.int64))          # the whole plane's own row-major list
    p = xc.products(ch.img, ch.seeds, levels=xc.TIER_B_LEVELS, weights=ch.weights, want_lists=False)
    assert (ch.labels() == p.labels).all() and (ch.stamps() == p.stamps).all() and (ch.final() == p.final).all()
    for L in xc.TIER_B_LEVELS:
        assert (ch.plane(L) == p.planes[L]).all() and (ch.plane(L, merging=False) == p.seg_planes[L]).all()
    assert (ch.tree() == p.tree).all()
    mt.check_invariants(p.tree[:, 0], p.tree[:, 1], p.tree[:, 2], p.tree[:, 3])
    assert ls.mismatch(ch.stats(), p.stats) is None, ls.mismatch(ch.stats(), p.stats)
    p8 = xc.products(ch.img, ch.seeds, weights=ch.weights8, want_lists=False)
    assert ch.weights8.dtype == np.uint8 and ls.mismatch(ch.stats(u8=True), p8.stats) is None, ls.mismatch(ch.stats(u8=True), p8.stats)


def test_the_wall_on_a_pieces_first_line_is_needed():
    """Without it a piece's first line is an ordinary border line of the piece alone but an interior line of the chain."""
    ch = xc.Chain((3 * xc.P + 57, 4))
    img = ch.img.copy()
    img[xc.P, :] = 7
    assert not np.array_equal(ol.segment_arrival(img, ch.seeds), ol.segment_arrival(ch.img, ch.seeds))


@pytest.mark.parametrize("shape", xc.TIER_B, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tier_b_patterns_flood_and_stay_far_from_the_ring_limit(shape):
    lines, short = max(shape), min(shape)
    n_full, rem = divmod(lines, xc.P)
    assert lines > 1 << 24 and (1 << 24) % xc.P == 144 and n_full * xc.P < 1 << 24 < lines          # the remainder straddles 2^24
    for grid in (64, 128, 256):          # the pieces' first lines meet every phase of the tile grids
        assert np.unique((np.arange(n_full) * xc.P) % grid).size == grid
    assert set(xc.order(n_full, xc.N_PATTERNS).tolist()) == {0, 2, 3, 4}          # a quadratic order: 4 of the 7 patterns, never periodic in P
    ch = xc.Chain((20 * xc.P + rem, short) if shape[0] > shape[1] else (short, 20 * xc.P + rem))          # the same patterns and remainder
    wrapped = xc.order(n_full, xc.N_PATTERNS)[0]
    assert not np.array_equal(ch.pat_img[wrapped][:70] if ch.tall else ch.pat_img[wrapped][:, :70],
                              ch.pat_img[-1][144:214] if ch.tall else ch.pat_img[-1][:, 144:214])          # lines past 2^24 differ from lines 0 .. 69
    for k, p in enumerate(ch.pat):
        assert len(p.ps) >= 1, k
        assert np.count_nonzero(p.labels) > len(p.ps), k                   # it floods beyond its seeds
        assert (p.tree[1:, 1] != mt.ALIVE).any(), k                      # lakes merge inside it
        assert p.max_rings < 1 << 12                                      # the ring limit is 2^24 - 1


def test_a_full_size_chain_lists_the_planes_own_maxima():
    """The seed list of a 2^24-line plane is the plane's own find_local_minima, in row-major order, tall and wide."""
    for shape in (xc.TIER_B[1], xc.TIER_B[3]):
        ch = xc.Chain(shape)
        assert ch.img.shape == shape and ch.n_seeds > 1 << 20
        assert np.array_equal(ch.seeds, ol.find_local_minima(ch.img).astype(np.int64))


@pytest.mark.parametrize("shape", xc.TIER_A, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tier_a_inputs_colour_what_their_interior_allows(shape):
    """Every interior pixel of an 8-, 5- or 3-wide plane floods (0.75 / 0.60 / 0.33 of the pixels); a plane of one or two lines
    has no interior and keeps its two seeds; with edge correction all of those are interior."""
    h, w = shape
    img, seeds = xc.tier_a_input(shape)
    labels, keys = ol.segment_arrival(img, seeds, want_keys=True)
    interior = max(h - 2, 0) * max(w - 2, 0)
    assert max(h, w) > 1 << 16 and (max(h, w) + 3) // 4 > 65535 or max(h, w) == 70001
    assert np.count_nonzero(labels) == (interior if interior else 2)
    if interior:
        assert len(seeds) > 1000 and len(np.unique(labels)) == len(seeds) + 1
        assert round(interior / (h * w), 2) == {8: 0.75, 5: 0.60, 3: 0.33}[min(h, w)]
    else:
        padded = ol.segment_arrival(img, seeds, edge=True)
        assert np.count_nonzero(padded) > h * w // 2
    stamps = xc.pack_stamps(keys)
    assert int((stamps[stamps != xc.KEY_INF] & 0xFFFFFF).max(initial=0)) < 1 << 12


def test_tier_c_slices_differ_and_the_cube_stacks():
    n, h, w = xc.TIER_C
    c = xc.Cube(n=40)
    assert n > 65535 and (h * w) % 128 == 0 and w % 4 == 0 and n * h * w < (1 << 31)          # one group: more than 65535 slices in it
    assert len(set(xc.order(n, xc.N_DISTINCT).tolist())) == 9          # a quadratic order reaches (17 + 1) / 2 of the slices
    assert (c.n_seeds_of >= 1).all() and all(int(f.max()) <= xc.TIER_C_MAX_LEVEL for f in c.imgs)
    for a in range(xc.N_DISTINCT):
        for b in range(a):
            assert not np.array_equal(c.distinct[a].labels, c.distinct[b].labels), (a, b)
            assert not np.array_equal(c.distinct[a].planes[7], c.distinct[b].planes[7]), (a, b)          # (at level 15 every slice is one lake)
    # the cube's layout is the slices' own products one after the other
    counts, rec, unc = c.lists(True)
    levels = xc.TIER_C_MAX_LEVEL + 1
    assert counts.shape == (40 * levels,) and counts.sum() == len(rec)
    for k in (0, 1, 39):
        p = c.distinct[c.which[k]]
        assert np.array_equal(c.cube[k], c.imgs[c.which[k]]) and np.array_equal(c.seeds[c.offsets[k]:c.offsets[k + 1]], p.ps)
        want = xc.products(c.cube[k], p.ps, max_level=xc.TIER_C_MAX_LEVEL)
        lo = int(counts[:k * levels].sum())
        for L in range(levels):
            cols, areas, u = want.lakes[L]
            assert unc[k * levels + L] == u and np.array_equal(rec[lo:lo + len(cols), 0], cols) and np.array_equal(rec[lo:lo + len(cols), 1], areas)
            lo += len(cols)
