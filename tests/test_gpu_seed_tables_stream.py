"""The seed tables built in list order (k_seed_tables_stream, csrc/ws_kernels.hip), -m gpu: every case compares final labels
with the CPU oracle (ol.segment_arrival) through the public segmenting calls on a FRESH context, then walks the context
through its forms the way tests/test_gpu_seed_regimes.py does: the shuffled twin of the list is refused by the tables and
repeated painted (the oracle's labels for the twin), and the list itself follows twice.

seed_tables() takes the list-order kernel for n * STREAM_PX_PER_SEED >= H * W (n > 0) and k_seed_tables below that; the
constants below restate csrc/ws_kernels.hip.  A wave of the new kernel owns the STREAM_E list entries [i0, i0 + STREAM_E), a
mask word belongs to the window that holds the word's first seed, a run of empty words to the window that holds the next
seed; the words go through an LDS row of STREAM_ROW words, and aligned chunks of STREAM_BIG empty words are left to the
plane waves of the same launch.  The cases put a window boundary, a row boundary and a chunk at each place where that can go
wrong.  The tables themselves are buffers of the context that no public call hands out, so there is no route to guard words
behind them (tests/test_gpu_seed_regimes.py has none either): the bad lists are checked through the labels, the error and
the context's next transform only.
"""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import oracle_lib as ol
import seed_cases as sc

pytestmark = pytest.mark.gpu

STREAM_E = 1024               # list entries per wave
STREAM_ROW = 512              # words of a wave's LDS row
STREAM_BIG = 4096             # words of a chunk that a plane wave fills
STREAM_PX_PER_SEED = 16       # the rule: the list-order kernel for one seed per this many pixels, or denser
W = 2048


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def dev(pkg):
    return importlib.import_module("rustronomy_watershed_amd.device")


def _to_dev(eng, img, seeds):
    import torch
    t_img = torch.from_numpy(np.ascontiguousarray(img)).to(eng.device)
    t_seeds = torch.from_numpy(np.asarray(seeds, dtype=np.int64).reshape(-1, 2).astype(np.int32)).to(eng.device).contiguous()
    return t_img, t_seeds


def _np32(t):
    return t.cpu().numpy().view(np.uint32)


def _stream(n, npx):
    return n > 0 and n * STREAM_PX_PER_SEED >= npx


def _walk(dev, img, px, want_stream=True, twin="shuffled"):
    """One fresh context: the list, its twin (refused, repeated painted), the list twice more."""
    h, w = img.shape
    px = np.asarray(px, dtype=np.int64)
    assert (np.diff(px) > 0).all() and px[0] >= 0 and px[-1] < h * w
    assert _stream(len(px), h * w) == want_stream, (len(px), h * w)
    seeds = sc.from_pixels(px, w)
    want = ol.segment_arrival(img, seeds)
    eng = dev.DeviceEngine(0)

    def run(s):
        t_img, t_seeds = _to_dev(eng, img, s)
        return _np32(eng.segment(t_img, t_seeds))

    got = run(seeds)
    assert got.shape == want.shape and (got == want).all(), ("fresh context", int((got != want).sum()))
    if twin == "shuffled":
        tw = sc.shuffled(seeds, 7)
    else:      # one entry twice, at the first window boundary if the list is that long
        k = min(STREAM_E - 1, len(seeds) - 1)
        tw = np.ascontiguousarray(np.concatenate([seeds[:k + 1], seeds[k:]]))
    want_tw = ol.segment_arrival(img, tw)
    got = run(tw)
    assert (got == want_tw).all(), ("twin", twin, int((got != want_tw).sum()))
    for tag in ("after the twin", "prediction flipped back"):
        got = run(seeds)
        assert (got == want).all(), (tag, int((got != want).sum()))


def _img(h, w, k):
    return sc.image(sc.KINDS[k % 3], h, w, 4000 + k)


def _bernoulli_px(lo, hi, density, seed):
    """Sorted pixel indices in [lo, hi)."""
    return lo + np.flatnonzero(np.random.default_rng(seed).random(max(hi - lo, 0)) < density)


def _around_a_word(h, before, bits, seed, density=0.25):
    """Exactly `before` seeds in the words below word WQ, then the seeds `bits` of word WQ, then a dense rest: entry `before`
    of the list is the first of `bits`."""
    wq = 600      # 19 200 pixels before it
    rng = np.random.default_rng(seed)
    head = np.sort(rng.choice(32 * wq, size=before, replace=False))
    rest = _bernoulli_px(32 * (wq + 1), h * W, density, seed + 1)
    return np.concatenate([head, 32 * wq + np.asarray(bits, dtype=np.int64), rest])


E = STREAM_E
BOUNDARY = [
    # (name, entries before the word, bits of the word): the window boundary lies between entries E - 1 and E
    ("straddle_after_first", E - 1, [3, 17]),                          # entries E - 1 and E in one word; the boundary after its first seed
    ("straddle_before_last", E - 3, [1, 5, 9, 30]),                    # ... and before its last
    ("straddle_middle", E - 2, [0, 8, 16, 31]),
    ("full_word_1_31", E - 1, list(range(32))),                        # 32 seeds in one word: 1 / 31 over two windows
    ("full_word_31_1", E - 31, list(range(32))),                       # ... and 31 / 1
    ("window_opens_a_word", E, [0, 4]),                                # entry E is the first seed of its word
    ("window_opens_a_word_at_bit_31", E, [31]),
    ("window_closes_a_word", E - 2, [6, 31]),                          # entry E - 1 is the last seed of its word
]


@pytest.mark.parametrize("case", BOUNDARY, ids=[c[0] for c in BOUNDARY])
def test_mask_word_at_a_window_boundary(dev, case):
    name, before, bits = case
    h = 64
    px = _around_a_word(h, before, bits, 100 + before)
    assert px[before] // 32 == 600 and px[before - 1] // 32 < 600
    assert (px[E - 1] // 32 == px[E] // 32) == (before < E < before + len(bits))
    _walk(dev, _img(h, W, before), px)


H_N = 7       # a plane small enough that a list of STREAM_E - 1 entries is above the rule (14 336 pixels)
N_CASES = [E - 1, E, E + 1, 2 * E, 2 * E + 1, 3 * E - 1]


@pytest.mark.parametrize("n", N_CASES)
def test_list_lengths_around_a_window(dev, n):
    px = np.sort(np.random.default_rng(n).choice(H_N * W, size=n, replace=False))
    _walk(dev, _img(H_N, W, n), px, twin="duplicate")


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("h", [64, 130])
def test_list_lengths_around_the_rule(dev, h, delta):
    thr = -(-h * W // STREAM_PX_PER_SEED)      # the smallest n of the list-order kernel on this plane
    n = thr + delta
    px = np.sort(np.random.default_rng(h + delta).choice(h * W, size=n, replace=False))
    _walk(dev, _img(h, W, h + delta), px, want_stream=delta >= 0, twin="duplicate")


@pytest.mark.parametrize("per_seed", [2, 9])
def test_dense_random_lists(dev, per_seed):
    h = 66
    px = _bernoulli_px(0, h * W, 1.0 / per_seed, per_seed)
    assert len(px) > 10 * E
    _walk(dev, _img(h, W, per_seed), px)


def test_width_that_is_no_multiple_of_a_word(dev):
    h, w = 65, 2084      # W % 32 != 0, W % 4 == 0: words run across the ends of the rows
    px = _bernoulli_px(0, h * w, 0.2, 5)
    px = np.union1d(px, [h * w - 1, h * w - 5])      # the last, short word holds seeds
    assert (h * w) % 32 and _stream(len(px), h * w)
    seeds_img = _img(h, w, 5)
    _walk(dev, seeds_img, px)


def test_empty_run_longer_than_the_row_inside_a_window(dev):
    h = 64      # 4096 words
    # the run starts 300 entries into a window: words [w0, w0 + 2.5 rows)
    head = _bernoulli_px(0, 32 * 1500, 0.25, 1)
    head = head[: 3 * E + 300]
    w0 = int(head[-1]) // 32 + 1
    px = np.concatenate([head, _bernoulli_px(32 * (w0 + 5 * STREAM_ROW // 2), h * W, 0.25, 2)])
    assert len(px) > 3 * E + 300 + E
    _walk(dev, _img(h, W, 1), px)


@pytest.mark.parametrize("where", ["start", "end", "both"])
def test_empty_run_at_the_ends_of_the_plane(dev, where):
    h = 64
    lo = 700 if where in ("start", "both") else 0                   # more than a row of empty words before the first seed
    hi = 4096 - (900 if where in ("end", "both") else 0)            # ... and behind the last
    px = _bernoulli_px(32 * lo + 5, 32 * hi - 7, 0.3, lo + hi)
    _walk(dev, _img(h, W, lo + hi), px)


def test_empty_run_that_holds_a_whole_plane_wave_chunk(dev):
    h = 130      # 8320 words: every pixel of words [0, 520) and [8300, 8320) a seed, nothing between -- the aligned chunk
    px = np.concatenate([np.arange(0, 32 * 520), np.arange(32 * 8300, h * W)])      # [4096, 8192) lies inside one run
    assert _stream(len(px), h * W) and 520 < STREAM_BIG and 8300 > 2 * STREAM_BIG
    _walk(dev, _img(h, W, 2), px)


def test_empty_runs_across_several_plane_wave_chunks_and_seeds_in_one_of_them(dev):
    h = 130      # chunk 0 holds seeds only in its first words, chunk 1 one dense stretch in its middle, chunk 2 (short) the end
    px = np.concatenate([np.arange(0, 32 * 300), np.arange(32 * 6000, 32 * 6300), np.arange(32 * 8310, h * W)])
    assert _stream(len(px), h * W)
    _walk(dev, _img(h, W, 3), px)


# ---- a seed at the last pixel of a word, the next word empty and first of a 64-pixel tile column: the resolve's halo seeds read
# `first` from that empty word (its base must be the number of seeds before it)

@pytest.mark.parametrize("rows", [(63, 64, 65), (0, 1, 127, 128, 129)], ids=["tile_row_1", "plane_edges_and_tile_row_2"])
def test_halo_seed_beside_an_empty_word(dev, rows):
    h = 130
    m = np.random.default_rng(rows[0]).random((h, W)) < 0.2
    for r in rows:
        for j in (1, 7, 16, 27):
            # left side of tile column j: the seed is its left halo pixel (column 64 j - 1, bit 31), the tile's first word is empty
            m[r, 64 * j - 32:64 * j + 32] = False
            m[r, 64 * j - 1] = True
            # right side of tile column j + 2: the seed is its right halo pixel (column 64 (j + 3), bit 0), the tile's last word is empty
            m[r, 64 * (j + 3) - 32:64 * (j + 3) + 32] = False
            m[r, 64 * (j + 3)] = True
    px = np.flatnonzero(m.reshape(-1))
    _walk(dev, _img(h, W, rows[0]), px)


# ---- a stack of slices, slice_first; a row block, colour_bias

def test_stack_of_three_slices_with_an_empty_one(dev):
    import torch
    h = 40
    eng = dev.DeviceEngine(0)
    imgs = [_img(h, W, 10 + k) for k in range(3)]
    pxs = [_bernoulli_px(0, h * W, 0.25, 21), np.zeros(0, dtype=np.int64), _bernoulli_px(0, h * W, 0.2, 23)]
    lists = [sc.from_pixels(p, W) for p in pxs]
    n = sum(len(p) for p in pxs)
    assert len(pxs[0]) % STREAM_E not in (0, STREAM_E - 1) and _stream(n, 3 * h * W) and (h * W) % 128 == 0      # the boundary inside a window
    offs = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    cube = torch.from_numpy(np.stack(imgs)).to(eng.device)
    allseeds = torch.from_numpy(np.concatenate(lists).astype(np.int32)).to(eng.device).contiguous()
    for rep in range(2):
        got = _np32(eng.segment_batch(cube, allseeds, offs))
        for k in range(3):
            assert (got[k] == ol.segment_arrival(imgs[k], lists[k])).all(), (rep, k)
    assert not got[1].any()
    # the twin: slice 2's list shuffled
    lists_tw = [lists[0], lists[1], sc.shuffled(lists[2], 3)]
    alltw = torch.from_numpy(np.concatenate(lists_tw).astype(np.int32)).to(eng.device).contiguous()
    got = _np32(eng.segment_batch(cube, alltw, offs))
    for k in range(3):
        assert (got[k] == ol.segment_arrival(imgs[k], lists_tw[k])).all(), ("twin", k)
    got = _np32(eng.segment_batch(cube, allseeds, offs))
    for k in range(3):
        assert (got[k] == ol.segment_arrival(imgs[k], lists[k])).all(), ("after the twin", k)


def test_row_blocks_of_two_ranks(pkg):
    ffi = pkg._ffi
    g = importlib.import_module("rustronomy_watershed_amd.group").Group.local(2)
    try:
        h = 128
        img = np.ascontiguousarray(_img(h, W, 30))
        px = _bernoulli_px(0, h * W, 0.2, 31)
        seeds = sc.from_pixels(px, W)

        def run(s):
            s = np.ascontiguousarray(np.asarray(s, dtype=np.uint64).reshape(-1, 2))
            out = np.full((h, W), 7, dtype=np.uint64)
            opt = ffi.Options(254)
            rounds = ctypes.c_uint32(0)
            rc = ffi.lib().ws_segment_tiled(g._h, img.ctypes.data, h, W, W, s.ctypes.data, len(s), ctypes.byref(opt), 0, out.ctypes.data,
                                            ctypes.byref(rounds))
            assert rc == 0, (rc, ffi.lib().ws_group_last_error(g._h))
            return out

        want = ol.segment_arrival(img, seeds)
        assert (run(seeds) == want).all()
        tw = sc.shuffled(seeds, 5)
        assert (run(tw) == ol.segment_arrival(img, tw)).all()
        assert (run(seeds) == want).all()
    finally:
        g.close()


# ---- lists that the walk must refuse

def _bad_base(h):
    px = _bernoulli_px(0, h * W, 0.25, 77)
    assert len(px) > 4 * E
    return sc.from_pixels(px, W)


BAD_ORDER = ["duplicate_at_the_boundary", "descending_across_the_boundary", "duplicate_inside_a_window", "window_swapped_with_the_next"]


@pytest.mark.parametrize("name", BAD_ORDER)
def test_lists_that_are_not_strictly_increasing_are_painted(dev, name):
    h = 64
    base = _bad_base(h)
    img = _img(h, W, 40)
    bad = {
        "duplicate_at_the_boundary": np.concatenate([base[:E], base[E - 1:]]),                              # entries E - 1 and E equal
        "descending_across_the_boundary": np.concatenate([base[:E - 1], base[E:E + 1], base[E - 1:E], base[E + 1:]]),
        "duplicate_inside_a_window": np.concatenate([base[:E + 500], base[E + 499:]]),
        "window_swapped_with_the_next": np.concatenate([base[:E], base[2 * E:3 * E], base[E:2 * E], base[3 * E:]]),
    }[name]
    bad = np.ascontiguousarray(bad)
    eng = dev.DeviceEngine(0)

    def run(s):
        t_img, t_seeds = _to_dev(eng, img, s)
        return _np32(eng.segment(t_img, t_seeds))

    want = ol.segment_arrival(img, base)
    assert (run(base) == want).all()
    got, want_bad = run(bad), ol.segment_arrival(img, bad)
    assert (got == want_bad).all(), (name, int((got != want_bad).sum()))
    assert (run(base) == want).all() and (run(base) == want).all()


@pytest.mark.parametrize("at", [E + 400, E + 5, E - 1, E, 0], ids=["middle_of_a_window", "look_ahead_entry", "last_of_a_window",
                                                                   "first_of_a_window", "first_of_the_list"])
@pytest.mark.parametrize("what", ["row", "column"])
def test_a_seed_outside_the_plane_is_an_error(pkg, dev, at, what):
    h = 64
    base = _bad_base(h)
    img = _img(h, W, 41)
    bad = base.copy()
    if what == "row":
        bad[at, 0] = h + 3
    else:
        bad[at, 1] = W + 1
    eng = dev.DeviceEngine(0)

    def run(s):
        t_img, t_seeds = _to_dev(eng, img, s)
        return _np32(eng.segment(t_img, t_seeds))

    want = ol.segment_arrival(img, base)
    assert (run(base) == want).all()
    with pytest.raises(IndexError):
        run(bad)
    assert (run(base) == want).all()      # the context works on
