"""The round recipes of the seam-repair flow (run with -m gpu): pass 0 on 256 x 64 tiles (k_relax0_tall) runs one full round
(sweeps down, right, up, then the checked sweep left) and from the second round on one free sweep up in front of the checked
sweep; the bands (k_relax, SEAM 1) do the same from their second round on, the 64-row strips keep their full rounds.

The flow is forced at small sizes with set_seam_repair_min_pixels(1); labels AND arrival stamps are compared pixel for pixel
with the CPU oracle, and with what the same context gives at the default threshold (the alternating grids).  Shapes are
(H, W).  Noise at 300 x 520 and 70 x 772 (shapes of tests/relax_plan_cases.txt) and at 130 x 512: a ragged last tile row, a
band at row 64 and at row 128.  A serpentine corridor with one seed, whose flood runs left to right, climbs, runs right to
left, climbs ... (and, flipped, descends): it travels for many rounds in the directions the later rounds no longer sweep
freely; six rounds cannot carry it through a tile, so tiles stop at their round cap and are finished by the re-runs of pass 2
and later, which the transform's statistics must show.  A smooth field of correlation 64 px, with the same check.  Stacks of
three slices, whose walls lie inside a lane's eight rows (labels only: a context keeps no stamps of a stack).  And 2048 x 2048
noise, where the flow's tile runs must not exceed what the recipes before this change needed -- the property the change
exists for."""
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import oracle_lib as ol

pytestmark = pytest.mark.gpu

# stats()["tiles_run_relax"] of ONE transform of cases.field(2048, 2048, 91) with the seam flow forced, measured on an MI355X with
# the library of the commit before the recipes changed (full rounds 1 and 2, then the checked sweep alone in pass 0; full rounds
# in bands and strips), five transforms in a row in one process: 686 each time (256 x 32 tile runs: pass 0 is 512 of them, a band a
# quarter, a 64-row strip slice two; the rest are the re-runs of pass 2 and later).  With the recipes of this file's docstring
# the same five transforms gave 670 each time: a figure that drifts back towards 686 says the recipes have stopped paying.
PARENT_TILES_RUN_2048 = 686


@pytest.fixture(scope="module")
def eng():
    ge.build_hip()
    ge.load_package()
    dev = importlib.import_module("rustronomy_watershed_amd.device")
    return dev.DeviceEngine(0)


def _pack(keys64):
    """The oracle's stamps (level << 32 | ring, ~0 for "never") in the engine's form (level << 24 | ring, KEY_INF and up)."""
    never = keys64 == np.uint64(0xFFFFFFFFFFFFFFFF)
    return ((keys64 >> np.uint64(32)) << np.uint64(24)) | (keys64 & np.uint64(0xFFFFFF)), never


def _same_stamps(got, want64):
    packed, never = _pack(want64)
    got = got.astype(np.uint64)
    return bool((got[~never] == packed[~never]).all() and (got[never] >= 0xFF000000).all())


def _run(eng, img, seeds):
    import torch
    d_img = torch.from_numpy(np.ascontiguousarray(img)).to(eng.device)
    d_seeds = torch.from_numpy(np.asarray(seeds, dtype=np.int64).reshape(-1, 2).astype(np.int32)).to(eng.device).contiguous()
    labels = eng.segment(d_img, d_seeds).cpu().numpy().view(np.uint32)
    stamps = eng.last_arrival().cpu().numpy().view(np.uint32)
    return labels, stamps


def _check(eng, img, seeds):
    """Returns the statistics of the transform that took the seam flow."""
    want, want_keys = ol.segment_arrival(img, np.asarray(seeds, dtype=np.uint64).reshape(-1, 2), want_keys=True)
    eng.ctx.set_seam_repair_min_pixels(1)
    eng.ctx.set_profiling(True)
    try:
        labels, stamps = _run(eng, img, seeds)
        st = eng.stats()
    finally:
        eng.ctx.set_profiling(False)
        eng.ctx.set_seam_repair_min_pixels(0)
    assert labels.shape == want.shape and (labels == want).all()
    assert _same_stamps(stamps, want_keys)
    old_labels, old_stamps = _run(eng, img, seeds)      # the default threshold: no seam repair at this size
    assert (old_labels == labels).all() and (old_stamps == stamps).all()
    return st


def _assert_reruns(st, h, w):
    # Pass 0 runs every 256 x 32 tile of the plane once (tiles_run_relax counts in those units, a tall tile as two); bands and
    # strips together cover a fraction of the plane, fewer units than that.  Whatever exceeds twice the plane's tiles was run by
    # pass 2 and later: tiles that pass 0, a band or a slice gave up on at its round cap, or that a neighbour flagged.
    tiles = ((w + 255) // 256) * ((h + 31) // 32)
    print(f"relax passes {st['relax_passes']}, tile runs {st['tiles_run_relax']} on {tiles} tiles, rounds {st['relax_tile_iterations']}")
    assert st["relax_passes"] >= 3 and st["tiles_run_relax"] > 2 * tiles, (st["relax_passes"], st["tiles_run_relax"], tiles)


@pytest.mark.parametrize("shape", [(300, 520), (70, 772), (130, 512)])
def test_noise_fields_labels_and_stamps(eng, shape):
    img = cases.field(*shape, 91)
    _check(eng, img, ol.find_local_minima(img))


def serpentine(h, w, pitch=6):
    """Walls (255: never flooded) with one corridor of level 7, a pixel wide: along row h - 3 from left to right, `pitch` rows
    up at the right end, back from right to left, up at the left end, ...  Returns the image and the corridor's first pixel."""
    img = np.full((h, w), 255, dtype=np.uint8)
    rows = list(range(h - 3, 1, -pitch))
    for k, r in enumerate(rows):
        img[r, 2:w - 2] = 7
        if k + 1 < len(rows):
            c = w - 3 if k % 2 == 0 else 2
            img[rows[k + 1]:r, c] = 7
    return img, (h - 3, 2)


@pytest.mark.parametrize("flipped", [False, True])
def test_serpentine_corridor_with_one_seed(eng, flipped):
    img, (r, c) = serpentine(300, 520)
    if flipped:      # the same corridor from the top: the flood descends
        img, r = np.ascontiguousarray(img[::-1]), 300 - 1 - r
    assert img[r, c] == 7
    want = ol.segment_arrival(img, np.array([[r, c]], dtype=np.uint64))
    assert (want[img == 7] == 1).all()      # the flood reaches the corridor's far end
    _assert_reruns(_check(eng, img, np.array([[r, c]], dtype=np.uint64)), 300, 520)


def test_smooth_field_of_correlation_64_px(eng):
    img = cases.smooth_field(300, 520, 92, octaves=5)      # the coarsest octave has a knot every 64 px
    seeds = ol.find_local_minima(img)
    assert len(seeds) >= 1
    _assert_reruns(_check(eng, img, seeds), 300, 520)


@pytest.mark.parametrize("s,h,w", [(3, 96, 256), (3, 100, 512)])
def test_stacks_of_three_slices(eng, s, h, w):
    # 96 rows, 256 wide: one tile column -- such a stack keeps the alternating grids; 100 rows, 512 wide takes the flow, and
    # its walls (rows 99 | 100, 199 | 200) lie inside a lane's eight rows and inside a band.  Labels only: a context keeps no
    # stamps of a stack to hand out.
    import torch
    himgs = [cases.field(h, w, 93 + k) if k % 2 == 0 else cases.smooth_field(h, w, 93 + k) for k in range(s)]
    hseeds = [np.asarray(ol.find_local_minima(a), dtype=np.int64).reshape(-1, 2) for a in himgs]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in hseeds])])
    cube = torch.from_numpy(np.stack(himgs)).to(eng.device)
    allseeds = torch.from_numpy(np.concatenate(hseeds)).to(torch.int32).to(eng.device).contiguous()
    want = [ol.segment_arrival(himgs[k], hseeds[k].astype(np.uint64)) for k in range(s)]
    got = {}
    for min_px in (1, 0):
        eng.ctx.set_seam_repair_min_pixels(min_px)
        try:
            labels = eng.segment_batch(cube, allseeds, offs).cpu().numpy().view(np.uint32)
        finally:
            eng.ctx.set_seam_repair_min_pixels(0)
        for k in range(s):
            assert (labels[k] == want[k]).all(), (min_px, k)
        got[min_px] = labels
    assert (got[0] == got[1]).all()


def tiles_run_2048(eng):
    """One transform of the 2048 x 2048 noise field with the seam flow forced: labels and stats()["tiles_run_relax"]."""
    import torch
    img = cases.field(2048, 2048, 91)
    seeds = np.asarray(ol.find_local_minima(img), dtype=np.int64).reshape(-1, 2)
    d_img = torch.from_numpy(img).to(eng.device)
    d_seeds = torch.from_numpy(seeds.astype(np.int32)).to(eng.device).contiguous()
    eng.ctx.set_seam_repair_min_pixels(1)
    eng.ctx.set_profiling(True)
    try:
        labels = eng.segment(d_img, d_seeds).cpu().numpy().view(np.uint32)
        st = eng.stats()
    finally:
        eng.ctx.set_profiling(False)
        eng.ctx.set_seam_repair_min_pixels(0)
    return img, seeds, labels, int(st["tiles_run_relax"])


def test_noise_2048_labels_and_no_more_tile_runs_than_before(eng):
    img, seeds, labels, runs = tiles_run_2048(eng)
    want = ol.segment_arrival(img, seeds.astype(np.uint64))
    print(f"tiles_run_relax {runs} (before the recipes changed: {PARENT_TILES_RUN_2048})")
    assert (labels == want).all()
    assert runs <= PARENT_TILES_RUN_2048, (runs, PARENT_TILES_RUN_2048)
