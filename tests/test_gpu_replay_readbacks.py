"""The read-backs of a replayed transform (csrc/ws_segment.hip, run_fused_form): the lookahead pass's convergence slot and
the error words reach the host's pinned mirror from block 0 of k_resolve_chase (ResolveJob::read_back), ahead of that
kernel's early returns, instead of from a launch of their own.

Three calls with identical buffers: the second captures the graph, the third replays it.  The third call's contents are
what each case is about; it runs as one call and as its segment_begin / segment_end halves."""
import functools
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import oracle_lib as ol

H, W = 130, 132


@functools.lru_cache(maxsize=None)
def noise_case():
    img = cases.field(H, W, 21)
    seeds = np.ascontiguousarray(np.asarray(ol.find_local_minima(img), dtype=np.uint64).reshape(-1, 2))
    return img, seeds, ol.segment(img, seeds)


@functools.lru_cache(maxsize=None)
def serpent_case():
    """256 x 256, one seed, one level: walls every 16 columns with gaps alternating top and bottom, so that the flood runs
    down one band and up the next and crosses the relaxation's tile seams some fifty times, one after the other."""
    img = np.full((256, 256), 9, dtype=np.uint8)
    for k, x in enumerate(range(16, 256, 16)):
        img[:, x] = 255
        gap = slice(1, 4) if k % 2 else slice(252, 255)
        img[gap, x] = 9
    seeds = np.array([[2, 2]], dtype=np.uint64)
    want = ol.segment(img, seeds)
    assert (want[1:-1, 1:-1][img[1:-1, 1:-1] == 9] == 1).all()      # the flood reaches every band
    return img, seeds, want


@pytest.fixture(scope="module")
def dev():
    ge.build_hip()
    ge.load_package()
    return importlib.import_module("rustronomy_watershed_amd.device")


def _replayed(dev, img, first, third, form, passes_only=False):
    """Two calls with the list `first`, then `third` written into the same buffer and a third call: (labels, stats) of it."""
    import torch
    with torch.cuda.stream(torch.cuda.Stream(0)):      # (the legacy null stream cannot be captured)
        eng = dev.DeviceEngine(0)
        if passes_only:      # the passes themselves: with one seed the default would end inside the graph, through the tile queue
            assert ge.load_package()._ffi.lib().ws_ctx_set_persistent_pass(eng.ctx.handle, 0) == 0
        d_img = torch.from_numpy(np.ascontiguousarray(img)).to(eng.device)
        d_seeds = torch.from_numpy(first.astype(np.int64).astype(np.int32)).to(eng.device).contiguous()
        out = torch.zeros(img.shape, dtype=torch.int32, device=eng.device)
        for _ in range(2):
            eng.segment(d_img, d_seeds, out=out)
        assert third.shape == first.shape
        d_seeds.copy_(torch.from_numpy(third.astype(np.int64).astype(np.int32)))
        out.zero_()
        torch.cuda.synchronize()
        try:
            if form == "call":
                eng.segment(d_img, d_seeds, out=out)
            else:
                eng.segment_begin(d_img, d_seeds, out)
                eng.segment_end()
        finally:
            stats = eng.stats()
            assert stats["graph_launches"] == 1, stats
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint32), stats


FORMS = ["call", "begin_end"]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_unchanged_contents(dev, form):
    img, seeds, want = noise_case()
    got, _ = _replayed(dev, img, seeds, seeds, form)
    assert (got == want).all(), int((got != want).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_a_seed_outside_the_plane_is_reported_by_that_very_call(dev, form):
    img, seeds, _ = noise_case()
    bad = seeds.copy()
    bad[len(bad) // 2] = (H + 3, 5)
    pkg = ge.load_package()
    with pytest.raises(pkg.SeedOutOfBounds):
        _replayed(dev, img, seeds, bad, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_a_list_that_is_no_longer_strictly_increasing_is_repeated_with_painted_labels(dev, form):
    img, seeds, _ = noise_case()
    swapped = seeds.copy()
    k = len(seeds) // 3
    swapped[[k, k + 7]] = seeds[[k + 7, k]]
    got, _ = _replayed(dev, img, seeds, swapped, form)
    want = ol.segment(img, swapped)
    assert (got == want).all(), int((got != want).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_a_flood_that_outlasts_the_graphs_passes_still_sends_its_slot(dev, form):
    img, seeds, want = serpent_case()
    got, stats = _replayed(dev, img, seeds, seeds, form, passes_only=True)
    assert stats["relax_passes"] > 5, stats      # the gate was closed: the host read the slot and went on with the loop
    assert (got == want).all(), int((got != want).sum())
