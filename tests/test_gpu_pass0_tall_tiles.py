"""Pass 0 of the seam-repair flow on 256 x 64 tiles (k_relax0_tall) and the bands astride every 64th row (run with -m gpu).

The flow is forced at small sizes with set_seam_repair_min_pixels(1); labels AND arrival stamps are compared pixel for pixel
with the CPU oracle, and with what the same context gives at the default threshold (the 256 x 32 path).  Shapes are (H, W):
one tile, several, ragged in both directions (W % 4 == 0, H no multiple of 64 or 32), a last tile half empty with a seam at
row 64 but none at row 32, stacks whose slice walls fall inside a tile and exactly on a seam, a smooth field on which pass 0
stops at its round cap (both 256 x 32 tiles of a tile are marked for their re-run), one seed, a seed in every other pixel,
a lower maximum water level, and a replayed graph.  (Stacks: labels only -- a context keeps no stamps of a stack to hand out.)"""
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import oracle_lib as ol

pytestmark = pytest.mark.gpu


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
    old_labels, old_stamps = _run(eng, img, seeds, max_level)      # the default threshold: the 256 x 32 path
    assert (old_labels == labels).all() and (old_stamps == stamps).all()


@pytest.mark.parametrize("shape", [(64, 256), (128, 512), (200, 260), (72, 1028), (96, 256),
                                   (96, 512), (65, 512), (136, 772)])      # (the last three: two tile columns, so that the flow applies, on the same heights)
def test_noise_fields_labels_and_stamps(eng, shape):
    img = cases.field(*shape, 61)
    _check(eng, img, ol.find_local_minima(img))


def test_smooth_field_on_which_pass0_stops_at_its_round_cap(eng):
    # correlation about 32 px: floods cross many patches, six rounds do not settle a tile; all minima, then three of them
    img = cases.smooth_field(256, 512, 7, octaves=4)
    seeds = ol.find_local_minima(img)
    _check(eng, img, seeds)
    _check(eng, img, seeds[:: max(len(seeds) // 3, 1)][:3])


def test_one_seed_and_a_seed_in_every_other_pixel(eng):
    img = cases.field(136, 520, 62)
    _check(eng, img, np.array([[70, 300]], dtype=np.uint64))
    rr, cc = np.meshgrid(np.arange(136, dtype=np.uint64), np.arange(520, dtype=np.uint64), indexing="ij")
    pick = (rr + cc) % 2 == 0
    _check(eng, img, np.stack([rr[pick], cc[pick]], axis=1))      # row-major, strictly increasing; border pixels among them


@pytest.mark.parametrize("max_level", [1, 100, 253])
def test_max_water_level_below_254(eng, max_level):
    img = cases.field(200, 260, 63)
    _check(eng, img, ol.find_local_minima(img), max_level)


@pytest.mark.parametrize("s,h,w", [(3, 40, 512), (5, 64, 512)])
def test_stacks_of_slices(eng, s, h, w):
    # slice walls inside a 256 x 64 tile (40 rows) and exactly on its seams (64 rows), through the batch entry point.
    # Labels only: the context does not hand out the stamps of a stack (ws_last_arrival_device: "no arrival stamps").
    import torch
    himgs = [cases.field(h, w, 80 + k) if k % 2 == 0 else cases.smooth_field(h, w, 80 + k) for k in range(s)]
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


def test_replayed_graph_with_the_same_buffers():
    # the same context and buffers three times and more: from the third call on the first passes are a replayed graph
    import torch
    ge.build_hip()
    ge.load_package()
    dev = importlib.import_module("rustronomy_watershed_amd.device")
    with torch.cuda.stream(torch.cuda.Stream()):      # capture is not allowed on the legacy null stream
        e = dev.DeviceEngine(0)
        h, w = 200, 520
        imgs = [cases.field(h, w, 64), cases.smooth_field(h, w, 65)]
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
