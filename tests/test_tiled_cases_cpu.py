"""The inputs of tests/tiled_cases.py reach the regimes they are made for -- proved on the CPU oracle alone (ol.segment_arrival,
ol.merge_arrival), so that an edit to a generator cannot quietly empty tests/test_gpu_tiled_edges.py -- and the row-block
protocol of rustronomy-watershed_amd/distributed.py computes them right on the numpy stand-in for the block steps
(tests/numpy_engine.py) over gloo: if a GPU test fails on one of these cases, this tells the protocol apart from a kernel."""
import os
import tempfile

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import __graft_entry__ as ge
import oracle_lib as ol
import tiled_cases as tc
from test_distributed_cpu import _free_port


def _ids(cases):
    return [c[0] for c in cases]


def _blocks(h, world):
    return [tc.tile_rows(h, r, world) for r in range(world)]


# ---- the forms ---------------------------------------------------------------------------------------------------------------

def test_every_case_has_the_form_its_name_says():
    names = set()
    for name, img, seeds, world in tc.all_cases():
        assert name not in names
        names.add(name)
        edge, shift = tc.edge_options(name)
        e = 2 if edge else 0
        ph, pw = img.shape[0] + e, img.shape[1] + e
        assert img.dtype == np.uint8 and ph >= world and world in (2, 3, 4, 8)
        s = np.asarray(seeds, dtype=np.int64).reshape(-1, 2)
        lim_r, lim_c = (img.shape if shift else (ph, pw))
        assert len(s) and (s >= 0).all() and (s[:, 0] < lim_r).all() and (s[:, 1] < lim_c).all()
        form = tc.form_of(name)
        if form == "fast":
            assert pw % 4 == 0 and tc.is_strictly_increasing(s, pw), name
        elif form == "wide":
            assert pw % 4 != 0 and tc.is_strictly_increasing(s, pw), name
        elif form == "shuffled":
            assert (np.diff(s[:, 0]) < 0).any() and len(np.unique(s, axis=0)) == len(s), name      # rows out of order: explicit colours
        else:
            assert not tc.is_strictly_increasing(s, pw) and len(np.unique(s, axis=0)) == len(s) - 1, name
    assert {n.split("/")[0] for n in names} == set("abcdefg")


def test_twins_are_the_same_field():
    by = {c[0]: c for c in tc.all_cases()}
    for name, (_, img, seeds, world) in by.items():
        if tc.form_of(name) != "fast":
            continue
        stem = name[: -len("fast")]
        twins = [by[stem + f] for f in ("shuffled", "wide") if stem + f in by]
        assert twins, name
        for tname, timg, tseeds, tworld in twins:
            assert tworld == world
            if tc.form_of(tname) == "wide":
                assert (timg[:, :-1] == img).all() and (timg[:, -1] == 255).all() and (tseeds == seeds).all()
            else:
                assert (timg == img).all() and (np.unique(tseeds, axis=0) == seeds).all()


# ---- a, b: thin blocks ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("letter", ["a", "b"])
def test_thin_blocks_own_one_or_two_rows(letter):
    # every rank owns 1 or 2 rows.  A rank that owns exactly one row AND has two halo rows is a middle rank, so a group of two has
    # none, and the 2 * world rows of family b give every rank two: per world >= 3, the family holds such a case (family a: every case)
    thin_middle = {}
    for name, img, seeds, world in tc.family(letter):
        owned = [r1 - r0 for r0, r1, _, _ in _blocks(img.shape[0], world)]
        assert set(owned) <= {1, 2}, name
        has = any(r1 - r0 == 1 and hi - lo == 3 for r0, r1, lo, hi in _blocks(img.shape[0], world))
        thin_middle[world] = thin_middle.get(world, False) or has
        if letter == "a":
            assert set(owned) == {1} and has == (world >= 3), name
        else:
            assert img.shape[0] in (world + 1, 2 * world - 1, 2 * world)
    assert all(thin_middle[w] for w in (3, 4, 8)) and not thin_middle[2]
    if letter == "b":      # some ranks own one row, others two
        assert any(len({r1 - r0 for r0, r1, _, _ in _blocks(img.shape[0], world)}) == 2 for _, img, _, world in tc.family("b"))


# ---- c: seam seeds -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.family("c"), ids=_ids(tc.family("c")))
def test_seam_seeds_sit_on_seam_and_halo_rows(case):
    name, img, seeds, world = case
    h, w = img.shape
    assert (h, w) == tc.SEAM_SHAPE
    rows_with_seed = set(int(r) for r in np.asarray(seeds)[:, 0])
    variant = name.split("/")[1]
    blocks = _blocks(h, world)
    if variant in ("seams", "astride"):
        for r0, r1, lo, hi in blocks:
            for r in {r0, r1 - 1, lo, hi - 1}:      # first and last owned row, and the halo rows (the neighbours' seam rows)
                assert r in rows_with_seed, (name, r)
            for r in (r0, r1 - 1):
                assert {(r, c) for c in (0, 1, w - 2, w - 1)} <= {tuple(int(v) for v in s) for s in np.asarray(seeds)}
    if variant == "astride":
        have = {tuple(int(v) for v in s) for s in np.asarray(seeds)}
        for r0, r1, _, _ in blocks[1:]:
            assert {(r0 - 1, 30), (r0, 30), (r0 - 1, 31), (r0, 31)} <= have
    if variant == "empty_rank1":
        _, _, lo, hi = blocks[1]
        assert 0 < 1 < world - 1 and not any(lo <= r < hi for r in rows_with_seed)
        assert {lo - 1, hi} <= rows_with_seed              # ... and the floods start right outside it
    if variant == "last_rank_only":
        r0, r1, _, _ = blocks[-1]
        assert all(r0 <= r < r1 for r in rows_with_seed)
    # every rank's owned rows hold a colour all the same: the floods reach the ranks that have no seed
    want = ol.segment_arrival(img, seeds)
    for r0, r1, _, _ in blocks:
        assert want[r0:r1].any(), name


# ---- d: zigzag -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.family("d"), ids=_ids(tc.family("d")))
def test_zigzag_crosses_every_seam_forty_times(case):
    name, img, seeds, world = case
    labels, keys = ol.segment_arrival(img, seeds, want_keys=True)
    k = keys.astype(np.int64)                         # (level << 32 | ring): one ring apart is a difference of one
    for r0, r1, _, _ in _blocks(img.shape[0], world)[:-1]:
        both = (labels[r1 - 1] != 0) & (labels[r1] != 0)
        crossings = int((both & (np.abs(k[r1 - 1] - k[r1]) == 1)).sum())
        assert crossings >= 40, (name, r1, crossings)
    up = (k[1:] < k[:-1])[:-1][labels[1:-1] != 0].any()
    assert up                                          # ... in both directions: somewhere the flood climbs


# ---- e: plateau ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.family("e"), ids=_ids(tc.family("e")))
def test_plateau_takes_thirty_rings(case):
    name, img, seeds, world = case
    labels, keys = ol.segment_arrival(img, seeds, want_keys=True)
    rings = keys[labels != 0] & np.uint64(0xFFFFFFFF)
    assert int(rings.max()) >= 30, name
    assert img.shape[0] == 33 and world in (3, 4)


# ---- f: linked lakes -------------------------------------------------------------------------------------------------------------

def _components(mask):
    """Number of 4-connected components of a small boolean plane."""
    mask = mask.copy()
    n = 0
    h, w = mask.shape
    for r in range(h):
        for c in range(w):
            if not mask[r, c]:
                continue
            n += 1
            stack = [(r, c)]
            mask[r, c] = False
            while stack:
                y, x = stack.pop()
                for yy, xx in ((y + 1, x), (y - 1, x), (y, x + 1), (y, x - 1)):
                    if 0 <= yy < h and 0 <= xx < w and mask[yy, xx]:
                        mask[yy, xx] = False
                        stack.append((yy, xx))
    return n


def _lakes(merged, h, world):
    """{lake id: blocks whose owned rows it touches}"""
    out = {}
    for i in np.unique(merged):
        if i:
            rows = np.unique(np.nonzero(merged == i)[0])
            out[int(i)] = sorted({k for k, (r0, r1, _, _) in enumerate(_blocks(h, world)) if ((rows >= r0) & (rows < r1)).any()})
    return out


@pytest.mark.parametrize("case", tc.family("f"), ids=_ids(tc.family("f")))
def test_linked_lakes_reach_their_regimes(case):
    name, img, seeds, world = case
    h = img.shape[0]
    assert (h, img.shape[1] - (tc.form_of(name) == "wide"), world) in tc.LINKED_SHAPES
    blocks = _blocks(h, world)
    top = ol.merge_arrival(img, seeds, max_level=254)
    lakes = _lakes(top, h, world)
    assert len(lakes) >= 2
    if h == 8:
        assert any(len(b) >= 6 for b in lakes.values()), lakes
    else:
        assert min(r1 - r0 for r0, r1, _, _ in blocks) >= 3
        # the blocks that hold a flooded row are all of them here; a lake that touches every one ...
        spanning = [i for i, b in lakes.items() if b == list(range(world))]
        assert spanning
        ok = False
        for i in spanning:
            # ... in two pieces or more inside every middle block (joined only through the other blocks) ...
            pieces = [_components(top[r0:r1] == i) for r0, r1, _, _ in blocks[1:-1]]
            # ... whose id is a seed in the interior of a block that is not block 0: neither an owned boundary row nor a halo row
            row = int(np.asarray(seeds)[i - 1, 0])
            k = next(k for k, (r0, r1, _, _) in enumerate(blocks) if r0 <= row < r1)
            r0, r1, _, _ = blocks[k]
            ok |= min(pieces) >= 2 and k != 0 and r0 < row < r1 - 1
        assert ok, (name, lakes)
        # ... and it passes through a rank that holds none of its seeds: block 0 has no seed at all
        assert not (np.asarray(seeds)[:, 0] < blocks[0][1]).any()
        low = _lakes(ol.merge_arrival(img, seeds, max_level=60), h, world)
        assert len(low) >= 4, low
        assert any(len(b) == 1 for b in low.values()) and any(len(b) > 1 for b in low.values()), low


# ---- g: edge correction ----------------------------------------------------------------------------------------------------------

def test_edge_cases_give_rank_0_the_ring_row_and_equal_their_padded_twins():
    seen_ring_only = False
    for name, img, seeds, world in tc.family("g"):
        edge, shift = tc.edge_options(name)
        assert edge
        ph = img.shape[0] + 2
        r0, r1, _, _ = tc.tile_rows(ph, 0, world)
        seen_ring_only |= (r0, r1) == (0, 1) and img.shape == (2, 32) and world == 4
        pad, moved = tc.padded_equivalent(img, seeds, shift)
        want = ol.segment_arrival(pad, moved)
        if not shift:
            assert (want == ol.segment(img, seeds, edge=True)).all(), name
        assert np.count_nonzero(want) > len(np.unique(np.asarray(seeds), axis=0)), name      # something floods
    assert seen_ring_only


# ---- the protocol on the numpy stand-in, over gloo ---------------------------------------------------------------------------------

def _protocol_worker(rank, world, port, jobs, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import importlib
        ge.load_package()
        wd = importlib.import_module("rustronomy_watershed_amd.distributed")
        from numpy_engine import NumpyBlockEngine
        for j, (img, seeds, max_level, merging) in enumerate(jobs):
            r0, r1, lo, hi = wd.row_block(img.shape[0], rank, world)
            loc, col = wd.local_seeds(seeds.astype(np.int64), lo, hi)
            block = NumpyBlockEngine(img[lo:hi], loc.numpy(), col.numpy(), max_level)
            if merging:
                owned, rounds = wd.merge_tiled(block, rank, world, lo, img.shape[0], len(seeds))
            else:
                owned, rounds = wd.segment_tiled(block, rank, world)
            assert owned.shape[0] == r1 - r0
            np.save(os.path.join(outdir, f"part{j}_{rank}.npy"), owned.numpy().view(np.uint32))
            np.save(os.path.join(outdir, f"rounds{j}_{rank}.npy"), np.array([rounds]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 4])
def test_protocol_on_the_numpy_engine_equals_the_oracle(world):
    # families c, d and f: segmenting, and merge_tiled for family f at its two levels (one process group per world, all cases in it)
    jobs, want, names = [], [], []
    for name, img, seeds, w in tc.all_cases("cdf"):
        if w != world:
            continue
        s = np.asarray(seeds, dtype=np.uint64).reshape(-1, 2)
        jobs.append((img, s, 254, False))
        want.append(ol.segment_arrival(img, s))
        names.append(name)
        if name.startswith("f/"):
            for lvl in tc.LINKED_LEVELS:
                jobs.append((img, s, lvl, True))
                want.append(ol.merge_arrival(img, s, max_level=lvl))
                names.append(f"{name}@merge{lvl}")
    assert jobs
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_protocol_worker, args=(world, _free_port(), jobs, d), nprocs=world, join=True)
        for j, name in enumerate(names):
            got = np.concatenate([np.load(os.path.join(d, f"part{j}_{r}.npy")) for r in range(world)], axis=0)
            rounds = {int(np.load(os.path.join(d, f"rounds{j}_{r}.npy"))[0]) for r in range(world)}
            assert len(rounds) == 1, name                  # every rank takes part in every exchange
            assert (got == want[j]).all(), (name, int((got != want[j]).sum()))
