"""k_resolve_local, seed tables on the 16-byte path (csrc/ws_resolve.hip, HALO_SEEDS): a halo cell that is a seed of the
plane holds the seed's colour, worked out from numbers the tile holds already, instead of a reference -- bit for bit
against the oracle (ol.segment; ol.merge_arrival for ws_merge_device).

  128 x 128        whole tiles, W % 32 == 0: a left halo pixel sits in the previous table word
  130 x 132        W % 4 == 0, rows start inside a table word, partial tiles
  66 x 1092        a tile column at x0 = 1024, where the word left of the tile starts another 128-byte line, and a second
                   tile row only two rows high
  61 x 67          the 4-byte path: unchanged references
  3 x 50 x 132     a stack of slices through ws_segment_batch_device.  50 * 132 is no
                   multiple of 128, so these slices run one by one (stackable, csrc/ws_batch.hip); they stay,
                   and ...
  3 x 96 x 132     ... is the stack that does run as ONE plane (96 * 132 = 99 * 128): tile rows straddle slice borders and
                   the top halo row of the tile row at 192 belongs to another slice (no tile row of 50-row slices starts on
                   a slice's first row either)

Seed lists: the image's local minima, and adversarial lists that are still strictly increasing (adversarial_lists).
The CPU half (not marked gpu) derives from the oracle's stamps alone that every noise case of the 16-byte path has chains
that end at a halo seed, and chains that leave through a halo pixel that is none, on each of the four sides: the GPU half
cannot pass on an input that misses the code."""
import functools
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import halo_seed_refs as hs
import oracle_lib as ol

TS = 64
# generator seeds picked on the CPU so that the counts of test_the_oracle_sends_chains_... hold
PLANES = {"128x128": (128, 128, 13), "130x132": (130, 132, 11), "66x1092": (66, 1092, 11), "61x67": (61, 67, 14)}
STACKS = {"3x50x132": (3, 50, 132, 15), "3x96x132": (3, 96, 132, 15)}
VEC_PLANES = ["128x128", "130x132", "66x1092"]


def _rc(pos, w):
    pos = np.unique(np.asarray(pos, dtype=np.int64))
    return np.ascontiguousarray(np.stack([pos // w, pos % w], axis=1).astype(np.uint64))


def _pos(rc, w):
    rc = np.asarray(rc, dtype=np.int64).reshape(-1, 2)
    return rc[:, 0] * w + rc[:, 1]


def adversarial_lists(h, w, minima, rows=None):
    """name -> (n, 2) seeds of an h x w plane, every list strictly increasing.  `rows`: the plane's rows that lie next to a
    horizontal tile seam (a slice of a stack passes its own)."""
    m = _pos(minima, w)
    ys, xs = np.mgrid[0:h, 0:w]
    flat = (ys * w + xs).ravel()
    seam_cols = [c for c in (63, 64) if c < w]
    seam_rows = [r for r in ((63, 64) if rows is None else rows) if r < h]
    on_seam = np.isin(xs.ravel(), seam_cols) | np.isin(ys.ravel(), seam_rows)
    out = {"seams": _rc(np.concatenate([m, flat[on_seam]]), w)}      # every pixel of columns 63, 64 and rows 63, 64 a seed
    if w > 64:
        # the list's first seed at (0, 63), the left halo of tile column 1; its last seed a right halo, (h - 2, 64)
        out["first_is_left_halo"] = _rc(np.concatenate([[63], m[m > 63]]), w)
        last = (h - 2) * w + 64
        out["last_is_right_halo"] = _rc(np.concatenate([m[m < last], [last]]), w)
    border = [(0, 63), (0, 64), (h - 1, 63), (h - 1, 64)] + [(r, c) for r in seam_rows for c in (0, w - 1)]
    border = [r * w + c for r, c in border if c < w]
    out["border_next_to_seams"] = _rc(np.concatenate([m, border]), w)
    for name, s in out.items():
        assert (np.diff(_pos(s, w)) > 0).all() and len(s) > 0, name
    return out


@functools.lru_cache(maxsize=None)
def plane_case(name):
    h, w, seed = PLANES[name]
    img = cases.field(h, w, seed)
    minima = np.ascontiguousarray(np.asarray(ol.find_local_minima(img), dtype=np.uint64).reshape(-1, 2))
    lists = {"minima": minima}
    if name in VEC_PLANES:
        lists.update(adversarial_lists(h, w, minima))
    return img, lists


@functools.lru_cache(maxsize=None)
def stack_case(name):
    s, h, w, seed = STACKS[name]
    imgs = [cases.field(h, w, seed + 100 * k) for k in range(s)]
    minima = [np.asarray(ol.find_local_minima(im), dtype=np.uint64).reshape(-1, 2) for im in imgs]
    lists = {"minima": minima}
    # the stacked plane's rows next to a tile seam, in each slice's own rows; and seeds on the slices' border rows
    seam_rows = [[r - k * h for r in range(TS - 1, s * h, TS) for r in (r, r + 1) if k * h <= r < (k + 1) * h] for k in range(s)]
    adv = [adversarial_lists(h, w, minima[k], rows=seam_rows[k]) for k in range(s)]
    for key in adv[0]:
        lists[key] = [adv[k][key] for k in range(s)]
    edge_rows = np.concatenate([np.arange(1, w - 1, 2), (h - 1) * w + np.arange(2, w - 1, 3)])
    lists["slice_border_rows"] = [_rc(np.concatenate([_pos(minima[k], w), edge_rows]), w) for k in range(s)]
    return imgs, lists


@functools.lru_cache(maxsize=None)
def want_plane(name, which, merging):
    img, lists = plane_case(name)
    return ol.merge_arrival(img, lists[which]) if merging else ol.segment(img, lists[which])


@functools.lru_cache(maxsize=None)
def want_stack(name, which):
    imgs, lists = stack_case(name)
    return np.stack([ol.segment(imgs[k], lists[which][k]) for k in range(len(imgs))])


def _shuffled(seeds, k):
    return np.ascontiguousarray(seeds[np.random.default_rng(k).permutation(len(seeds))])


# ---- CPU side ------------------------------------------------------------------------------------------------------------------

def _side_counts(keys):
    ch = hs.leaving_chains(keys)
    return {hs.SIDE_NAMES[s]: (int((ch["at_seed"] & (ch["side"] == s)).sum()),
                               int((ch["is_ref"] & ~ch["at_seed"] & (ch["side"] == s)).sum())) for s in range(4)}


def test_the_oracle_sends_chains_to_halo_seeds_and_past_them_on_every_side():
    for name in VEC_PLANES:
        img, lists = plane_case(name)
        h, w = img.shape
        assert w % 4 == 0
        _, keys = ol.segment_arrival(img, lists["minima"], want_keys=True)
        for side, (at_seed, past) in _side_counts(keys).items():
            assert at_seed >= 8 and past >= 1, (name, side, at_seed, past)
    assert 1024 % TS == 0 and 1024 + TS < 1092 and 1024 * 4 % 128 == 0 and 66 - TS == 2 and 67 % 4 != 0
    for name, (s, h, w, _) in STACKS.items():
        imgs, lists = stack_case(name)
        assert w % 4 == 0 and ((h * w) % 128 == 0) == (name == "3x96x132")      # only that one runs as one stacked plane
        per_slice = [ol.segment_arrival(imgs[k], lists["minima"][k], want_keys=True)[1] for k in range(s)]
        if (h * w) % 128 == 0:
            for side, (at_seed, past) in _side_counts(np.concatenate(per_slice)).items():
                assert at_seed >= 8 and past >= 1, (name, side, at_seed, past)
        else:      # every slice a plane of its own, one tile row high: chains leave to the left and right only
            for keys in per_slice:
                c = _side_counts(keys)
                assert h <= TS and c["U"] == c["D"] == (0, 0)
                assert all(c[side][0] >= 8 and c[side][1] >= 1 for side in "LR"), (name, c)
        straddle = [y0 for y0 in range(0, s * h, TS) if y0 // h != (min(y0 + TS, s * h) - 1) // h]
        assert straddle, name                                                   # tile rows straddle slice borders
        if name == "3x96x132":      # ... and the tile row at 192 starts on a slice's first row: its top halo row is another slice's
            assert [y0 for y0 in range(TS, s * h, TS) if (y0 - 1) // h != y0 // h] == [2 * h]


# ---- GPU side ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def eng(pkg):
    import torch
    with torch.cuda.stream(torch.cuda.Stream(0)):
        yield importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


def _np32(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def _dev(eng, img, seeds):
    import torch
    s = np.asarray(seeds, dtype=np.int64).reshape(-1, 2).astype(np.int32)
    return torch.from_numpy(np.ascontiguousarray(img)).to(eng.device), torch.from_numpy(s).to(eng.device).contiguous()


PLANE_LISTS = [(n, "minima") for n in PLANES] + [(n, k) for n in VEC_PLANES
                                                 for k in ("seams", "first_is_left_halo", "last_is_right_halo", "border_next_to_seams")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,which", PLANE_LISTS, ids=[f"{n}-{k}" for n, k in PLANE_LISTS])
def test_segment_with_halo_seed_colours(eng, name, which):
    img, lists = plane_case(name)
    got = _np32(eng.segment(*_dev(eng, img, lists[which])))
    want = want_plane(name, which, False)
    assert got.shape == want.shape and (got == want).all(), int((got != want).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["minima", "seams", "border_next_to_seams"])
@pytest.mark.parametrize("name", ["128x128", "130x132"])
def test_merge_takes_the_tile_colour_from_a_halo_seed(eng, name, which):
    img, lists = plane_case(name)
    got = _np32(eng.merge(*_dev(eng, img, lists[which])))
    want = want_plane(name, which, True)
    assert got.shape == want.shape and (got == want).all(), int((got != want).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("merging", [False, True], ids=["segment", "merge"])
@pytest.mark.parametrize("name", ["128x128", "130x132"])
def test_shuffled_list_keeps_painted_labels_and_references(eng, name, merging):
    img, lists = plane_case(name)
    seeds = _shuffled(lists["minima"], 5)
    assert (np.diff(_pos(seeds, img.shape[1])) <= 0).any()
    got = _np32((eng.merge if merging else eng.segment)(*_dev(eng, img, seeds)))
    want = ol.merge_arrival(img, seeds) if merging else ol.segment(img, seeds)
    assert (got == want).all(), int((got != want).sum())


STACK_LISTS = [(n, k) for n in STACKS for k in ("minima", "seams", "first_is_left_halo", "last_is_right_halo", "border_next_to_seams",
                                                "slice_border_rows")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,which", STACK_LISTS, ids=[f"{n}-{k}" for n, k in STACK_LISTS])
def test_stack_of_slices_with_halo_seed_colours(eng, name, which):
    import torch
    imgs, lists = stack_case(name)
    per = lists[which]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in per])])
    cube = torch.from_numpy(np.stack(imgs)).to(eng.device)
    allseeds = torch.from_numpy(np.concatenate(per).astype(np.int64).astype(np.int32)).to(eng.device).contiguous()
    got = _np32(eng.segment_batch(cube, allseeds, offs))
    stacked_launches = eng.stats()["launches_relax"]
    want = want_stack(name, which)
    assert got.shape == want.shape and (got == want).all(), int((got != want).sum())
    if name == "3x96x132":      # one transform for the stack: no more relaxation launches than one slice alone would make twice over
        one = eng.segment(*_dev(eng, imgs[0], per[0]))
        torch.cuda.synchronize()
        assert 0 < stacked_launches < 3 * eng.stats()["launches_relax"], (stacked_launches, eng.stats()["launches_relax"])
        assert (_np32(one) == want[0]).all()
