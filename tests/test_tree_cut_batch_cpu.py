"""Without a GPU: the cases of tests/tree_cut_batch_cases.py reach the regimes tests/test_gpu_tree_cut_batch.py names.  Everything
here is numpy over the CPU oracle's floods; the engine is not loaded."""
import numpy as np
import pytest

import tree_cut_batch_cases as bc
import tree_cut_catalogue_ref as cc

ALL = bc.STACKING + bc.LOOPING + bc.DEVICE_ONLY


def _outputs_differ(pa, pb, j):
    """Whether two slices' expected outputs for cut j differ: the plane, or the records measured over it."""
    if (pa[0][j] != pb[0][j]).any():
        return True
    ra, rb = pa[2][int(pa[3][j]):int(pa[3][j + 1])], pb[2][int(pb[3][j]):int(pb[3][j + 1])]
    return ra.shape != rb.shape or ra.tobytes() != rb.tobytes() or pa[5][j].tobytes() != pb[5][j].tobytes()


@pytest.mark.parametrize("name", ALL)
def test_slices_differ_for_every_cut(name):
    """A slice mix-up cannot pass: for every cut the expected outputs of any two slices with seeds differ -- the planes, except
    where a cut merges both slices into their first lake (a one-seed slice, merge_level 254), and there the records measured
    over them, since every slice has weights of its own.  For the first cut, which merges nothing, the planes themselves differ."""
    cube = bc.cube(name)
    per = cube.expected()
    seeded = [k for k, f in enumerate(cube.slices) if f.n_seeds]
    assert len(seeded) >= 2
    for j, cut in enumerate(cube.cuts):
        for a in seeded:
            for b in seeded:
                if a < b:
                    assert _outputs_differ(per[a], per[b], j), (name, cut, a, b)
                    if j == 0:
                        assert (per[a][0][j] != per[b][0][j]).any(), (name, cut, a, b)


def test_expected_layout_is_slice_major_then_cut():
    cube = bc.cube("9x8x16")
    lakes, region, offsets, hidden, hid = cube.expected_flat()
    k = len(cube.cuts)
    assert len(offsets) == cube.n_slices * k + 1 and len(hidden) == cube.n_slices * k == len(hid) and offsets[-1] == len(lakes) == len(region)
    per = cube.expected()
    for s in range(cube.n_slices):
        for j in range(k):
            lo, hi = int(offsets[s * k + j]), int(offsets[s * k + j + 1])
            assert (lakes[lo:hi] == per[s][1][int(per[s][3][j]):int(per[s][3][j + 1])]).all()
            assert (np.diff(lakes[lo:hi, 0].astype(np.int64)) > 0).all()      # increasing colour
            assert hidden[s * k + j] + lakes[lo:hi, 1].sum() == cube.plane_shape[0] * cube.plane_shape[1]
    assert cube.slices[1].n_seeds == 0 and cube.slices[2].n_seeds == 1      # a seedless and a one-seed slice


def test_runs_and_quads_hold_shown_pixels_of_two_slices():
    # 128-pixel planes: a 1024-pixel run holds eight slices and the ninth begins the next run
    small = bc.cube("9x8x16")
    assert small.plane_shape == (8, 16) and small.n_slices * 128 > bc.RUN == 8 * 128
    # 3840-pixel planes: runs straddle slices, with shown pixels on both sides
    mid = bc.cube("5x40x96")
    n = mid.plane_shape[0] * mid.plane_shape[1]
    assert n == 3840 and n % bc.RUN != 0
    flat = np.concatenate([p[0][0].ravel() for p in mid.expected()])
    both = 0
    for r in range(0, flat.size, bc.RUN):
        ks = np.arange(r, min(r + bc.RUN, flat.size)) // n
        shown = flat[r:r + bc.RUN] != 0
        both += len(set(ks[shown])) > 1
    assert both >= 1
    # 35-pixel planes: quads straddle slices with shown pixels of both, and slices lie off 16-byte alignment
    tiny = bc.cube("5x5x7")
    assert tiny.plane_shape == (5, 7) and [(35 * 4 * k) % 16 for k in range(1, 4)] == [12, 8, 4]
    flat = np.concatenate([p[0][0].ravel() for p in tiny.expected()])
    straddling = [q for q in range(0, flat.size - 3, 4) if q // 35 != (q + 3) // 35]
    assert any((flat[q:q + 4] != 0)[np.arange(q, q + 4) // 35 == q // 35].any() and (flat[q:q + 4] != 0)[np.arange(q, q + 4) // 35 != q // 35].any()
               for q in straddling)
    # the edge-corrected plane becomes 128 x 96; 130 x 98 does not stack (w % 4 != 0)
    assert bc.cube("6x126x94_edge").plane_shape == (128, 96) and bc.cube("5x130x98").plane_shape[1] % 4 != 0


@pytest.mark.parametrize("name", ["9x8x16", "5x40x96", "5x130x98", "5x5x7"])
def test_cuts_move_the_table_the_walk_and_both_and_meet_a_threshold_exactly(name):
    cube = bc.cube(name)
    cuts = cube.cuts
    a = cuts[1].min_area
    assert a > 0 and cuts[2].min_area == a + 1
    assert any(f.n_seeds and ((f.area[1:] == a) & (f.death[1:] != bc.ALIVE)).any() for f in cube.slices)      # met exactly by a dead node
    per = cube.expected()
    planes = lambda j: np.stack([p[0][j] for p in per])
    assert (planes(1) != planes(0)).any() or (planes(2) != planes(0)).any()      # thresholds alone: only the table moves
    assert (planes(2) != planes(1)).any() or name == "9x8x16" or name == "5x5x7"      # ... and a + 1 drops the node a kept
    assert (planes(3) != planes(0)).any() and (planes(4) != planes(0)).any()      # levels alone: only the walk moves
    assert (planes(5) != planes(1)).any()                                          # both
    assert sum(c.catalogue for c in cuts) == 2


def test_weights_are_u8_u16_and_none_and_sum_wr_passes_2_32_in_one_slice_only():
    kinds = {name: (None if bc.cube(name).weights is None else bc.cube(name).weights.dtype.name) for name in ALL}
    assert set(kinds.values()) == {None, "uint8", "uint16"}
    cube = bc.cube("5x130x98")
    top = []
    for p in cube.expected():
        recs = np.concatenate([p[2]["sum_wr"], p[5]["sum_wr"]])
        top.append(int(recs.max()))
    assert [t >= 1 << 32 for t in top] == [False, False, False, True, False], top


def test_thirty_two_cuts_with_repeats():
    cube = bc.cube("thirty_two")
    assert len(cube.cuts) == 32
    for pos, of in cc.REPEATS_32:
        assert cube.cuts[pos].key() == cube.cuts[of].key()
    assert len({c.key() for c in cube.cuts}) == 24


def test_checkerboard_fills_more_than_half_a_table_in_a_run():
    cube = bc.cube("checkerboard")
    assert all(f.n_seeds == 1024 for f in cube.slices)
    for p in cube.expected():
        assert min(cc.regions_per_run(p[0][0])) > 500      # of the 512 entries of the measuring table, the 2048 of the counting table


def test_chain_is_254_deep_in_one_slice_of_two():
    cube = bc.cube("chain")
    assert cube.n_slices == 2
    f = cube.slices[1]
    c, depth = f.n_seeds, 0
    while f.parent[c]:
        c, depth = int(f.parent[c]), depth + 1
    assert depth == 254


def test_tiled_cube_passes_the_grid_dimension_limit_from_three_distinct_slices():
    base, which, cuts = bc.tiled()
    assert len(which) == bc.TILED_SLICES > 65535 and set(which) == {0, 1, 2} and len(cuts) == 2
    per = base.expected(cuts)
    for j in range(2):
        assert (per[0][0][j] != per[1][0][j]).any() and (per[1][0][j] != per[2][0][j]).any() and (per[0][0][j] != per[2][0][j]).any()
    # consecutive slices differ: a shift by one slice cannot pass
    assert (which[1:] != which[:-1]).mean() > 0.5
    records = sum(f.n_seeds + 1 for f in base.slices) / 3 * bc.TILED_SLICES
    assert records * 2 * 4 < 64 << 20      # the counters of the whole cube are megabytes


def test_groups_of_two_two_and_one():
    """5 slices under a pixel limit of two planes: the seedless slice sits inside the first group, and every group ends with
    records, so the lists cross both group boundaries and a cap one short bites in the last group or the first."""
    cube = bc.cube("5x40x96")
    k = len(cube.cuts)
    offsets = cube.expected_flat()[2]
    ends = [int(offsets[2 * k]), int(offsets[4 * k]), int(offsets[5 * k])]
    assert cube.slices[1].n_seeds == 0 and 0 < ends[0] < ends[1] < ends[2]


def test_refusal_cases():
    cube = bc.cube("9x8x16")
    tree, first = cube.tree(), cube.first_records()
    assert bc.slice_verdict(cube, tree)
    # a record the whole array, read as one tree, accepts -- and its own slice does not
    i, p = bc.foreign_parent(cube)
    t = tree.copy()
    t[i, 0] = p
    k = max(s for s in range(cube.n_slices) if first[s] <= i)
    assert bc.record_ok(t, i) and not bc.record_ok(t, i, first[k]) and not bc.slice_verdict(cube, t)
    # a dead record with parent 0 in the last slice only
    last = cube.n_slices - 1
    dead = [c for c in range(1, cube.slices[last].n_seeds + 1) if tree[first[last] + c, 1] != bc.ALIVE]
    assert dead
    t = tree.copy()
    t[first[last] + dead[0], 0] = 0
    assert not bc.slice_verdict(cube, t)
    # a label n_k + 1 in a slice whose successor has more seeds: a valid record of the next slice
    ns = [f.n_seeds for f in cube.slices]
    ks = [s for s in range(cube.n_slices - 1) if 0 < ns[s] < ns[s + 1]]
    assert ks
    s = ks[0]
    assert first[s] + ns[s] + 1 == first[s + 1] < first[s + 2]
    assert ((cube.seg()[s] != 0) & (cube.keys()[s] >> 24 == 0)).any()      # a seed pixel, shown by every cut
