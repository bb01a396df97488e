"""The seam strips on 64-row slices (k_relax_strips_tall), which follow pass 0 on 256 x 64 tiles (GPU tests: run with -m gpu).

The flow is forced at small sizes with set_seam_repair_min_pixels(1); labels AND arrival stamps are compared pixel for pixel
with the CPU oracle, and with what the same context gives at the default threshold (the alternating grids).  Shapes are
(H, W), the smallest at which the kernel can go wrong: one seam and two full slices; a ragged last slice of 8 rows with two
seams and a ragged last tile column; a second slice of one row; a half slice; 34 seams (a second column of strip
workgroups) with a last tile column of 4 px; a seam whose right tile is 4 px wide; a smooth field on which slices stop at
their round cap (both tile rows on both sides of a seam are marked); a seed on a seam column at a slice end and a seed in
every other pixel; lower maximum water levels; stacks whose slice walls fall inside a strip slice, on its ends and on its
32-row half; a replayed graph.  (Stacks: labels only -- a context keeps no stamps of a stack to hand out.)"""
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import oracle_lib as ol

gpu = pytest.mark.gpu

NOISE_SHAPES = [(128, 512), (200, 772), (65, 512), (96, 512), (136, 8708), (192, 516)]
SMOOTH_SHAPE = (256, 512)
SEED_SHAPE = (136, 520)
LEVEL_SHAPE = (200, 772)
STACKS = [(3, 40, 512), (5, 64, 512), (3, 96, 512)]
GRAPH_SHAPE = (200, 520)


def test_every_shape_takes_the_seam_flow_and_the_tall_path():
    # relax_seam_flow (ws_relax_plan.hpp): two tile columns of 256, two tile rows of 32, a width that is a multiple of 4;
    # pass 0 on 256 x 64 tiles and the 64-row strips: more than 64 rows.  A stack is one plane of s * h rows.
    planes = NOISE_SHAPES + [SMOOTH_SHAPE, SEED_SHAPE, LEVEL_SHAPE, GRAPH_SHAPE] + [(s * h, w) for s, h, w in STACKS]
    for h, w in planes:
        ax, ay = (w + 255) // 256, (h + 31) // 32
        assert w % 4 == 0 and ax >= 2 and ay >= 2 and h > 64, (h, w)
    assert min(h for h, _ in planes) == 65      # the smallest height the tall path takes


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


def _run(eng, img, seeds, max_level=254):
    import torch
    d_img = torch.from_numpy(np.ascontiguousarray(img)).to(eng.device)
    d_seeds = torch.from_numpy(np.asarray(seeds, dtype=np.int64).reshape(-1, 2).astype(np.int32)).to(eng.device).contiguous()
    labels = eng.segment(d_img, d_seeds, max_level=max_level).cpu().numpy().view(np.uint32)
    stamps = eng.last_arrival().cpu().numpy().view(np.uint32)
    return labels, stamps


def _check(eng, img, seeds, max_level=254):
    want, want_keys = ol.segment_arrival(img, np.asarray(seeds, dtype=np.uint64).reshape(-1, 2), max_level=max_level, want_keys=True)
    eng.ctx.set_seam_repair_min_pixels(1)
    try:
        labels, stamps = _run(eng, img, seeds, max_level)
    finally:
        eng.ctx.set_seam_repair_min_pixels(0)
    assert labels.shape == want.shape and (labels == want).all()
    assert _same_stamps(stamps, want_keys)
    old_labels, old_stamps = _run(eng, img, seeds, max_level)      # the default threshold: no seam repair at this size
    assert (old_labels == labels).all() and (old_stamps == stamps).all()


@gpu
@pytest.mark.parametrize("shape", NOISE_SHAPES)
def test_noise_fields_labels_and_stamps(eng, shape):
    img = cases.field(*shape, 71)
    _check(eng, img, ol.find_local_minima(img))


@gpu
def test_smooth_field_on_which_slices_stop_at_their_round_cap(eng):
    # correlation about 32 px: floods cross many patches, four rounds do not settle a slice; all minima, then three of them
    img = cases.smooth_field(*SMOOTH_SHAPE, 7, octaves=4)
    seeds = ol.find_local_minima(img)
    _check(eng, img, seeds)
    _check(eng, img, seeds[:: max(len(seeds) // 3, 1)][:3])


@gpu
def test_a_seed_on_a_seam_column_at_a_slice_end_and_a_seed_in_every_other_pixel(eng):
    h, w = SEED_SHAPE
    img = cases.field(h, w, 72)
    _check(eng, img, np.array([[63, 256]], dtype=np.uint64))      # last row of the first slice, first column right of the seam
    rr, cc = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    pick = (rr + cc) % 2 == 0
    _check(eng, img, np.stack([rr[pick], cc[pick]], axis=1))      # row-major, strictly increasing; border pixels among them


@gpu
@pytest.mark.parametrize("max_level", [1, 100])
def test_max_water_level_below_254(eng, max_level):
    img = cases.field(*LEVEL_SHAPE, 73)
    _check(eng, img, ol.find_local_minima(img), max_level)


@gpu
@pytest.mark.parametrize("s,h,w", STACKS)
def test_stacks_of_slices(eng, s, h, w):
    # slice walls inside a 64-row strip slice (40 rows), exactly on its ends (64 rows) and on its 32-row half as well (96 rows),
    # through the batch entry point.  Labels only: the context does not hand out the stamps of a stack.
    import torch
    himgs = [cases.field(h, w, 90 + k) if k % 2 == 0 else cases.smooth_field(h, w, 90 + k) for k in range(s)]
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


@gpu
def test_replayed_graph_with_the_same_buffers():
    # the same context and buffers five times: from the third call on the first passes, strips included, are a replayed graph
    import torch
    ge.build_hip()
    ge.load_package()
    dev = importlib.import_module("rustronomy_watershed_amd.device")
    with torch.cuda.stream(torch.cuda.Stream()):      # capture is not allowed on the legacy null stream
        e = dev.DeviceEngine(0)
        h, w = GRAPH_SHAPE
        imgs = [cases.field(h, w, 74), cases.smooth_field(h, w, 75)]
        lists = [np.asarray(ol.find_local_minima(a), dtype=np.int64).reshape(-1, 2) for a in imgs]
        n = min(len(x) for x in lists)
        want = [ol.segment_arrival(imgs[k], lists[k][:n].astype(np.uint64), want_keys=True) for k in range(2)]
        d_img = torch.empty((h, w), dtype=torch.uint8, device=e.device)
        d_seeds = torch.empty((n, 2), dtype=torch.int32, device=e.device)
        out = torch.empty((h, w), dtype=torch.int32, device=e.device)
        e.ctx.set_seam_repair_min_pixels(1)
        try:
            replays = 0
            for rep in range(5):
                k = 0 if rep < 3 else 1      # three times the same contents, then other contents in the same buffers
                d_img.copy_(torch.from_numpy(imgs[k]))
                d_seeds.copy_(torch.from_numpy(lists[k][:n]).to(torch.int32))
                labels = e.segment(d_img, d_seeds, out=out).cpu().numpy().view(np.uint32)
                replays += e.stats()["graph_launches"]
                assert (labels == want[k][0]).all(), rep
                assert _same_stamps(e.last_arrival().cpu().numpy().view(np.uint32), want[k][1]), rep
            assert replays >= 2, replays
        finally:
            e.ctx.set_seam_repair_min_pixels(0)
