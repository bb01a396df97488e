"""The inputs of tests/tiled2d_cases.py reach the regimes they are made for -- proved on the CPU oracle alone (ol.segment_arrival
with its stamps, ol.merge_arrival), so that an edit to a generator cannot quietly empty tests/test_gpu_tiled2d_edges.py -- and
the 2-D protocol of rustronomy-watershed_amd/distributed.py computes them right on the numpy stand-in for the block steps
(tests/numpy_engine.py) over gloo: if a GPU test fails on one of these cases, this tells the protocol apart from a kernel.

The thin-tile proof of family u ("every tile owns one or two columns or rows") is asserted of the thin cases; the two u/uneven
cases (7 x 11 on (2, 3), 13 x 9 on (3, 2)) are there for tiles of unequal size and are held to that instead.  The protocol runs
on groups of at most four processes, so on the grids (2, 2) and (1, 4) only."""
import ctypes
import os
import tempfile

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import __graft_entry__ as ge
import oracle_lib as ol
import tiled_cases as tc
import tiled2d_cases as t2
from test_distributed_cpu import _free_port
from test_tiled_cases_cpu import _components

NEVER = np.uint64(0xFFFFFFFFFFFFFFFF)


def _ids(cases):
    return [c[0] for c in cases]


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


def _owned(shape, grid, rank):
    (r0, r1, _, _), (c0, c1, _, _) = t2.tile_grid(*shape, rank, *grid)
    return slice(r0, r1), slice(c0, c1)


# ---- the cut ------------------------------------------------------------------------------------------------------------------------

def test_the_seam_arithmetic_is_ws_tile_grid(pkg):
    L = pkg._ffi.lib()
    shapes = {(c[1].shape, g) for c in t2.all_cases("tuvwxy") for g in c[3]}
    shapes |= {((c[1].shape[0] + 2, c[1].shape[1] + 2), g) for c in t2.family("z") for g in c[3]}      # (the padded plane is what is cut)
    assert len(shapes) > 60
    for (h, w), (py, px) in sorted(shapes):
        covered = np.zeros((h, w), dtype=np.int64)
        for rank in range(py * px):
            rows, cols = (ctypes.c_size_t * 4)(), (ctypes.c_size_t * 4)()
            assert L.ws_tile_grid(h, w, rank, py, px, rows, cols) == 0, (h, w, py, px)
            assert (tuple(rows), tuple(cols)) == t2.tile_grid(h, w, rank, py, px), (h, w, py, px, rank)
            covered[rows[0]:rows[1], cols[0]:cols[1]] += 1
            assert t2.owner(h, w, py, px, rows[0], cols[0]) == rank == t2.owner(h, w, py, px, rows[1] - 1, cols[1] - 1)
        assert (covered == 1).all()
        # a split that does not divide gives the extra line to the first parts
        heights = [t2.tile_grid(h, w, k * px, py, px)[0][1] - t2.tile_grid(h, w, k * px, py, px)[0][0] for k in range(py)]
        assert heights == sorted(heights, reverse=True) and heights[0] - heights[-1] <= 1
    rows, cols = (ctypes.c_size_t * 4)(), (ctypes.c_size_t * 4)()
    assert L.ws_tile_grid(1, 64, 0, 2, 2, rows, cols) != 0      # fewer rows than tile rows


def test_every_case_is_well_formed():
    names = set()
    for name, img, seeds, grids in t2.all_cases():
        assert name not in names and grids
        names.add(name)
        assert img.dtype == np.uint8 and img.flags["C_CONTIGUOUS"]
        edge, shift = tc.edge_options(name)
        e = 2 if edge else 0
        s = np.asarray(seeds, dtype=np.int64).reshape(-1, 2)
        lim = img.shape if shift or not edge else (img.shape[0] + 2, img.shape[1] + 2)
        assert len(s) and (s >= 0).all() and (s[:, 0] < lim[0]).all() and (s[:, 1] < lim[1]).all(), name
        for py, px in grids:
            assert py * px <= 8 and py <= img.shape[0] + e and px <= img.shape[1] + e, name
    assert {n[0] for n in names} == set("tuvwxyz")


def test_the_transposed_family_holds_every_row_case_and_the_originals_of_a_b_d_e():
    by = {c[0]: c for c in t2.family("t")}
    for name, img, seeds, world in tc.all_cases("abcdef"):
        _, timg, tseeds, grids = by[f"t/T/{name}"]
        assert grids == [(1, world)] and (timg == img.T).all()
        assert sorted(map(tuple, tseeds.tolist())) == sorted((c, r) for r, c in np.asarray(seeds).tolist())
        if tc.form_of(name) in ("fast", "wide"):
            assert tc.is_strictly_increasing(tseeds, timg.shape[1]), name
        elif tc.form_of(name) == "dup":
            assert (tseeds[-1] == np.asarray(seeds)[-1][::-1]).all()      # the doubled entry is still the last
        assert (f"t/O/{name}" in by) == (name[0] in "abde")
        if name[0] in "abde":
            assert by[f"t/O/{name}"][3] == [(world, 1)] and (by[f"t/O/{name}"][1] == img).all()
    assert len(by) == len(tc.all_cases("abcdef")) + len(tc.all_cases("abde"))


# ---- u: thin tiles ------------------------------------------------------------------------------------------------------------------

def test_thin_tiles_own_one_or_two_columns_or_rows():
    held_widths, held_heights, grids = set(), set(), set()
    for name, img, seeds, [grid] in t2.family("u"):
        cut = t2.tiles(*img.shape, *grid)
        own_h = {r1 - r0 for (r0, r1, _, _), _ in cut}
        own_w = {c1 - c0 for _, (c0, c1, _, _) in cut}
        grids.add(grid)
        if "/uneven/" in name:
            assert len({(r1 - r0, c1 - c0) for (r0, r1, _, _), (c0, c1, _, _) in cut}) >= 2, name
            assert len({(hi - lo, chi - clo) for (_, _, lo, hi), (_, _, clo, chi) in cut}) >= 2, name
            continue
        if "/cols" in name:
            assert own_w <= {1, 2} and grid[0] == 1 and img.shape[0] in t2.THIN_LENGTHS, name
            held_widths |= {chi - clo for _, (_, _, clo, chi) in cut}
        elif "/rows" in name:
            assert own_h <= {1, 2} and grid[1] == 1 and img.shape[1] in t2.THIN_LENGTHS, name
            held_heights |= {hi - lo for (_, _, lo, hi), _ in cut}
        else:
            assert own_w <= {1, 2} and own_h <= {1, 2}, name
    # both sides of the w > 2 and h > 2 guards of the "no received ring differs" test
    assert {2, 3} <= held_widths and {2, 3} <= held_heights
    assert grids == {(1, p) for p in t2.THIN_PARTS} | {(p, 1) for p in t2.THIN_PARTS} | set(t2.THIN_GRIDS)
    assert {(c[1].shape, c[3][0]) for c in t2.family("u") if "/uneven/" in c[0]} == {((7, 11), (2, 3)), ((13, 9), (3, 2))}


# ---- v: seeds on crossings ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", t2.family("v"), ids=_ids(t2.family("v")))
def test_crossing_seeds_sit_where_ws_tile_grid_puts_the_seams(pkg, case):
    name, img, seeds, [grid] = case
    kind, g, special, dup_at = t2.V_SPECIAL[name]
    assert g == grid and img.shape == t2.CROSS_SHAPE and grid in t2.CROSS_GRIDS
    h, w = img.shape
    py, px = grid
    L = pkg._ffi.lib()
    place = []
    for rank in range(py * px):
        rows, cols = (ctypes.c_size_t * 4)(), (ctypes.c_size_t * 4)()
        assert L.ws_tile_grid(h, w, rank, py, px, rows, cols) == 0
        place.append((tuple(rows), tuple(cols)))
    have = {tuple(p) for p in np.asarray(seeds).tolist()}
    assert set(special) <= have
    if kind[0] in ("quad", "alone"):
        i, j = kind[1], kind[2]
        a, b = place[i * px + j], place[(i + 1) * px + j + 1]      # the tiles above-left and below-right of the crossing
        q = [(a[0][1] - 1, a[1][1] - 1), (a[0][1] - 1, b[1][0]), (b[0][0], a[1][1] - 1), (b[0][0], b[1][0])]
        assert b[0][0] == a[0][1] and b[1][0] == a[1][1]
        assert special == (q if kind[0] == "quad" else [q[kind[3]]])
        if kind[0] == "alone":
            assert len(have & set(q)) == 1
        # every quad pixel is owned by another tile and held by all four
        assert len({t2.owner(h, w, py, px, *p) for p in q}) == 4
        for k in (i * px + j, i * px + j + 1, (i + 1) * px + j, (i + 1) * px + j + 1):
            (_, _, lo, hi), (_, _, clo, chi) = place[k]
            assert all(lo <= r < hi and clo <= c < chi for r, c in q)
    elif kind[0] == "columns":
        want = set()
        for (r0, r1, lo, hi), (c0, c1, clo, chi) in place:      # every tile's halo columns and the owned columns next to them
            for c in ([clo, c0] if clo < c0 else []) + ([c1 - 1, chi - 1] if chi > c1 else []):
                want |= {(r, c) for r in range(h)}
        assert set(special) == want and len(want) == 2 * (px - 1) * h
    else:
        want = {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)}
        for (r0, r1, lo, hi), (c0, c1, clo, chi) in place:
            want |= {(r, c) for c in ({clo, c0} if clo < c0 else set()) | ({c1 - 1, chi - 1} if chi > c1 else set()) for r in (0, h - 1)}
            want |= {(r, c) for r in ({lo, r0} if lo < r0 else set()) | ({r1 - 1, hi - 1} if hi > r1 else set()) for c in (0, w - 1)}
        assert set(special) == want
    s = np.asarray(seeds, dtype=np.int64)
    labels = ol.segment_arrival(img, s)
    if kind[0] == "border":      # the field's border never floods: those pixels keep their painted colour
        for k, (r, c) in enumerate(s.tolist()):
            if (r, c) in want and dup_at is None:
                assert labels[r, c] == k + 1
    if name.endswith("/dup"):
        assert dup_at is not None and (s[-1] == s[dup_at]).all() and tuple(s[-1]) in set(special)
        assert labels[s[-1][0], s[-1][1]] == len(s)                   # the later entry's colour wins
        assert not (labels == dup_at + 1).any()
    elif name.endswith("/shuffled"):
        assert not tc.is_strictly_increasing(s, w) and len(have) == len(s)
    else:
        assert tc.is_strictly_increasing(s, w)
    assert np.count_nonzero(labels) > len(have)                        # something floods


# ---- w: corridors -------------------------------------------------------------------------------------------------------------------

def _walk_down(keys, far):
    """From the far end down the arrival stamps to the seed: every step to the one neighbour whose stamp is one ring less."""
    h, w = keys.shape
    path = [far]
    while keys[path[-1]] != 0:
        r, c = path[-1]
        k = int(keys[r, c])
        nxt = [(y, x) for y, x in ((r + 1, c), (r, c + 1), (r, c - 1), (r - 1, c))
               if 0 <= y < h and 0 <= x < w and keys[y, x] != NEVER and int(keys[y, x]) < k]
        assert len(nxt) == 1, (r, c, nxt)
        path.append(nxt[0])
    return path


@pytest.mark.parametrize("case", t2.family("w"), ids=_ids(t2.family("w")))
def test_corridors_cross_their_seams_K_times(case):
    name, img, seeds, grids = case
    assert set(np.unique(img)) == {t2.CORRIDOR_LEVEL, 255} and len(seeds) == 1
    open_ = img < 255
    nb = np.zeros(img.shape, dtype=np.int64)
    nb[1:] += open_[:-1]
    nb[:-1] += open_[1:]
    nb[:, 1:] += open_[:, :-1]
    nb[:, :-1] += open_[:, 1:]
    assert (nb[open_] <= 2).all() and (nb[open_] == 1).sum() == 2      # a path, and one path only
    labels, keys = ol.segment_arrival(img, seeds, want_keys=True)
    assert ((labels == 1) == open_).all()
    keys = keys.copy()
    keys[tuple(seeds[0])] = 0
    flooded = np.where(keys == NEVER, np.uint64(0), keys)
    far = tuple(int(v) for v in np.unravel_index(np.argmax(flooded), keys.shape))
    down = _walk_down(keys, far)
    assert down[::-1] == t2.W_PATH[name] and len(down) == int(open_.sum())
    assert int(keys[far] & np.uint64(0xFFFFFFFF)) == len(down) - 1       # a ring a pixel
    for grid in grids:
        seq = t2.crossings(down[::-1], img.shape, grid)
        K = t2.corridor_K(name, grid)
        assert K == len(seq), (name, grid)
        if "/serpentine/" in name:
            assert K >= 40 and grid[0] == 1
            own = t2.owner_plane(*img.shape, *grid)
            for cs in t2.seam_starts(img.shape[1], grid[1]):             # every column seam, 40 times
                assert int((open_[:, cs - 1] & open_[:, cs]).sum()) >= 40 and (own[:, cs - 1] != own[:, cs]).all()
        elif grid == (2, 2):
            assert K >= 24, (name, K)
            assert seq == ["col", "row"] * (K // 2) + ["col"] * (K % 2)  # row and column seams alternately
            visited = [t2.owner(*img.shape, 2, 2, *p) for p in down[::-1]]
            order = [k for n, k in enumerate(visited) if n == 0 or visited[n - 1] != k]
            assert order[:9] == [0, 1, 3, 2, 0, 1, 3, 2, 0]              # (0,0), (0,1), (1,1), (1,0), (0,0) ...
        else:
            assert grid == (1, 2) and set(seq) == {"col"} and K >= 24
    if img.shape == (70, 1100):      # a held plane spans several relaxation tiles of 256 columns
        assert grids == [(1, 2), (2, 2)] and t2.tile_grid(70, 1100, 0, 1, 2)[1][3] > 2 * 256
    turns = sum(1 for a, b, c in zip(down, down[1:], down[2:]) if (a[0] == b[0]) != (b[0] == c[0]))
    if "/spiral/" in name:
        assert turns >= 12 and turns >= K - 1


# ---- x: plateaus --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", t2.family("x"), ids=_ids(t2.family("x")))
def test_plateau_stamps_are_manhattan_distances_and_ties_fall_on_seams(case):
    name, img, seeds, grids = case
    h, w = img.shape
    assert (h, w) == t2.PLATEAU_SHAPE and (img == t2.PLATEAU_LEVEL).all()
    s = np.asarray(seeds, dtype=np.int64)
    labels, keys = ol.segment_arrival(img, s, want_keys=True)
    rr, cc = np.mgrid[0:h, 0:w]
    dist_ = np.min([np.abs(rr - r) + np.abs(cc - c) for r, c in s.tolist()], axis=0)
    inner = np.zeros((h, w), dtype=bool)
    inner[1:-1, 1:-1] = True
    inner[s[:, 0], s[:, 1]] = False
    assert (keys[inner] == ((np.uint64(t2.PLATEAU_LEVEL) << np.uint64(32)) | dist_[inner].astype(np.uint64))).all()
    edge = ~inner
    edge[s[:, 0], s[:, 1]] = False
    assert (keys[edge] == NEVER).all() and (labels[edge] == 0).all()      # the border never floods
    assert int(dist_[inner].max()) >= 40
    if len(s) == 1:
        assert (labels[inner] == 1).all()
        return
    k = np.where(keys == NEVER, np.uint64(1) << np.uint64(62), keys).astype(np.int64)
    k[s[:, 0], s[:, 1]] = 0
    for grid in grids:
        py, px = grid
        own = t2.owner_plane(h, w, py, px)
        on_seam = np.zeros((h, w), dtype=bool)
        for rs in t2.seam_starts(h, py):
            on_seam[rs - 1:rs + 1] = True
        on_col = np.zeros((h, w), dtype=bool)
        for cs in t2.seam_starts(w, px):
            on_col[:, cs - 1:cs + 1] = True
        found = {"row": 0, "col": 0}
        for r, c in zip(*np.nonzero((on_seam | on_col) & inner)):
            smaller = [(y, x) for y, x in ((r + 1, c), (r, c + 1), (r, c - 1), (r - 1, c)) if k[y, x] < k[r, c]]      # D, R, L, U
            assert smaller
            assert labels[r, c] == labels[smaller[0]], (name, r, c)
            if len({own[p] for p in smaller}) >= 2 and len({labels[p] for p in smaller}) == 2 and own[smaller[0]] != own[r, c]:
                # a tie between the two floods, parents in different tiles, and the winner lies in the other tile
                found["row" if on_seam[r, c] and smaller[0][0] != r else "col"] += 1
        assert found["col"] >= 1 and (found["row"] >= 1 or py == 1), (name, grid, found)


# ---- y: lakes linked through other tiles --------------------------------------------------------------------------------------------

def _reach(open_, start):
    seen = np.zeros(open_.shape, dtype=bool)
    stack = [start]
    seen[start] = True
    while stack:
        r, c = stack.pop()
        for y, x in ((r + 1, c), (r, c + 1), (r, c - 1), (r - 1, c)):
            if 0 <= y < open_.shape[0] and 0 <= x < open_.shape[1] and open_[y, x] and not seen[y, x]:
                seen[y, x] = True
                stack.append((y, x))
    return seen


@pytest.mark.parametrize("case", t2.family("y"), ids=_ids(t2.family("y")))
def test_linked_lakes_are_one_class_in_two_pieces_inside_the_named_tile(case):
    name, img, seeds, grids = case
    mask, tile, link = t2.Y_META[name]
    assert t2.merge_levels(name) == (link, link - 1, 254) and sorted(tile) == sorted(grids)
    assert _components(mask) == 1 and (img[mask] < 255).all() and int(img[mask].max()) == link
    for level in t2.merge_levels(name):
        merged = ol.merge_arrival(img, seeds, max_level=level)
        ids = np.unique(merged[mask])
        if level < link:      # not linked yet: the lake is still in pieces (or partly dry)
            assert len(ids) >= 2, (name, level)
            continue
        assert len(ids) == 1 and ids[0] != 0, (name, level, ids)
        lake = merged == ids[0]
        assert (lake == mask).all(), (name, level)
        for grid in grids:
            rows, cols = _owned(img.shape, grid, tile[grid])
            assert _components(lake[rows, cols]) >= 2, (name, level, grid)
    # merging, not one flood, makes it one class: the lake holds two seeds or more
    s = np.asarray(seeds, dtype=np.int64)
    assert int(mask[s[:, 0], s[:, 1]].sum()) >= 2
    own = t2.owner_plane(*img.shape, *grids[0])
    if name.startswith("y/corner"):
        assert grids == [(2, 2)] and set(own[s[:, 0], s[:, 1]].tolist()) == {0, 2}      # seeds in (0, 0) and (1, 0) only
        # the two basins: no path inside the union of tiles (0, 0), (1, 0) and (1, 1) ...
        seen = _reach((img < 255) & (own != 1), (3, 3))
        assert seen[5, 13] and not seen[19, 20] and not seen[18, 5]
        assert _reach(img < 255, (3, 3))[19, 20]                                          # ... but one through (0, 1)
        corridor = mask & (img == t2.LINK_LEVEL)
        assert (own[corridor] != 2).all() and (own[corridor] == 1).sum() > (own[corridor] != 1).sum()
        assert ol.merge_arrival(img, seeds)[18, 5] not in (0, ol.merge_arrival(img, seeds)[3, 3])      # (1, 0): a lake of its own
    if name.startswith("y/round_trip"):
        assert grids == [(2, 2)] and set(own[s[:, 0], s[:, 1]].tolist()) == {0}
        seq = t2.crossings(t2.walk(np.where(img == t2.LINK_LEVEL, 4, 255).astype(np.uint8), (3, 10)), img.shape, (2, 2))
        assert seq == ["col", "row", "col", "row"]      # out through the right seam, back in through the bottom one
    if name.startswith("y/linked"):
        assert grids[0][0] == 1 and not (own[s[:, 0], s[:, 1]] == 0).any()      # tile 0 holds no seed


# ---- z: edge correction -------------------------------------------------------------------------------------------------------------

def test_edge_cases_equal_their_padded_twins_and_a_tile_owns_only_the_ring_column():
    ring_only = False
    seen = set()
    for name, img, seeds, [grid] in t2.family("z"):
        edge, shift = tc.edge_options(name)
        assert edge
        seen.add((img.shape, grid, shift))
        pad, moved = tc.padded_equivalent(img, seeds, shift)
        want = ol.segment_arrival(pad, moved)
        assert (want == ol.segment(img, moved, edge=True)).all(), name          # (the oracle takes the list in plane coordinates)
        assert (ol.merge_arrival(pad, moved, max_level=120) == ol.merge_arrival(img, moved, max_level=120, edge=True)).all(), name
        assert (pad[1:-1, 1:-1] == img).all() and (moved >= 1).all() and (moved[:, 0] <= img.shape[0]).all() and (moved[:, 1] <= img.shape[1]).all()
        ph, pw = pad.shape
        for rank in range(grid[0] * grid[1]):
            _, (c0, c1, _, _) = t2.tile_grid(ph, pw, rank, *grid)
            ring_only |= img.shape[1] == 2 and set(range(c0, c1)) <= {0, pw - 1}
    assert ring_only
    assert seen == {((h, w), g, sh) for h, w, g in t2.EDGE_SHAPES for sh in (False, True)}
    assert {((2, 2), (2, 2)), ((6, 6), (2, 2)), ((6, 2), (2, 4))} == {(s, g) for s, g, _ in seen}


# ---- the protocol on the numpy stand-in, over gloo ----------------------------------------------------------------------------------

def _protocol2d_worker(rank, py, px, port, jobs, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=py * px)
    try:
        import importlib
        ge.load_package()
        wd = importlib.import_module("rustronomy_watershed_amd.distributed")
        from numpy_engine import NumpyBlockEngine
        for j, (img, seeds) in enumerate(jobs):
            (r0, r1, lo, hi), (c0, c1, clo, chi) = wd.tile_grid(img.shape[0], img.shape[1], rank, py, px)
            loc, col = wd.local_seeds2d(seeds.astype(np.int64), lo, hi, clo, chi)
            block = NumpyBlockEngine(img[lo:hi, clo:chi], loc.numpy(), col.numpy(), 254)
            labels, rounds = wd.segment_tiled2d(block, rank, py, px)
            np.save(os.path.join(outdir, f"part{j}_{rank}.npy"), labels.numpy().view(np.uint32)[r0 - lo:r1 - lo, c0 - clo:c1 - clo])
            np.save(os.path.join(outdir, f"rounds{j}_{rank}.npy"), np.array([rounds]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("py,px", [(2, 2), (1, 4)])
def test_2d_protocol_on_the_numpy_engine_equals_the_oracle(py, px):
    # families v and x, the corner link of y and the smallest spiral, on the grids of at most four tiles (one process group per
    # grid, all its cases in it)
    smallest = min((c for c in t2.family("w") if "/spiral/" in c[0]), key=lambda c: c[1].size)
    chosen = t2.family("v") + t2.family("x") + [c for c in t2.family("y") if c[0].startswith("y/corner")] + [smallest]
    jobs, names = [], []
    for name, img, seeds, grids in chosen:
        if (py, px) in grids:
            jobs.append((img, np.asarray(seeds, dtype=np.uint64).reshape(-1, 2)))
            names.append(name)
    assert jobs and {n[0] for n in names} == ({"v", "w", "x", "y"} if (py, px) == (2, 2) else {"x"})
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_protocol2d_worker, args=(py, px, _free_port(), jobs, d), nprocs=py * px, join=True)
        for j, name in enumerate(names):
            img, seeds = jobs[j]
            got = np.zeros(img.shape, dtype=np.uint32)
            rounds = set()
            for rank in range(py * px):
                rows, cols = _owned(img.shape, (py, px), rank)
                got[rows, cols] = np.load(os.path.join(d, f"part{j}_{rank}.npy"))
                rounds.add(int(np.load(os.path.join(d, f"rounds{j}_{rank}.npy"))[0]))
            assert len(rounds) == 1, name                      # every rank takes part in every exchange
            want = ol.segment_arrival(img, seeds)
            assert (got == want).all(), (name, int((got != want).sum()))
            if name[0] == "w":                                 # a stamp crosses one seam per exchange (test_gpu_tiled2d_edges.py)
                assert rounds.pop() >= t2.corridor_K(name, (py, px)) + 2
