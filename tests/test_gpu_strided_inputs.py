"""Device entry points on strided, offset and unaligned images (-m gpu).

Every image-taking call of include/ws_hip.h has a row_stride (cubes: a slice_stride too), and the kernels pick their code
by it.  Here every entry point is given a sub-rectangle of a larger device array (tests/strided.py): the pixels at
base + offset + y * row_stride + x, everything else -- guard bands, row gaps, slice gaps -- filled with 0x00 (ALWAYS_FILL: a
stray read floods early) and, in a second run, with 0xFF (NEVER_FILL: a stray read never floods).  Both runs must give the
CPU oracle's result for the COMPACT image, bit for bit, and leave the backing array as it was.

Which layout reaches which branch (a = the image pointer, s = row_stride; "al" = (a | s) % 4 == 0).  The guard band is a
multiple of 4 and torch's allocations are 256-byte aligned (asserted), so a % 4 == offset % 4.

  k_relax load phase (ws_relax.hip, `fast`), also the seam-repair shapes and the list / queue variants that share the test:
    al, s <= 2^32-1, W % 4 == 0, no edge corr.  dword fast path, every tile          PLANES rows 7, 10 (offset 0 / 64, s = w+4 / 2w)
    al, W % 4 != 0                              fast in tiles inside the image,       row 5 (w 1030, offset 64, pitch): 1030 > 4 tiles
                                                byte path in the last tile column
    a % 4 != 0 (any s), W % 4 == 0              byte path  (never run before)         rows 2 (w+2, offset 3), 9 (w+4, offset 2), 6
    a % 4 == 0, s % 4 != 0, W % 4 == 0          byte path  (never run before)         rows 3 (520, w+3), 8 (96, w+2)
    s > 2^32-1, al                              byte path                             test_row_stride_beyond_32_bits
    edge correction (padded_img_index)          byte path, every pixel through s      test_segment_* with edge=True, every row
    W < 4 (narrower than a patch)               byte path                             row 0 (w 3)
    seed_bits form / label-plane form           sorted list / shuffled list           test_segment_table_form / _painted_form
    SEAM shapes (bands, strips)                 al -> fast, else byte                 test_seam_repair_on_strided_planes (both)
    PERSIST queue (modes 1, 2), early sched (4) al -> queue taken; else the passes    test_persistent_pass_modes_on_strided_planes (both)
  flood_step (ws_kernels.hip):
    no padding, w % 4 == 0, al                  k_flood_step4                         ENGINE_SWEEP on rows 7, 10
    no padding, w % 4 == 0, not al              k_flood_step  (never run before)      ENGINE_SWEEP on rows 2, 3, 6, 8, 9
    w % 4 != 0, or edge correction              k_flood_step                          ENGINE_SWEEP on rows 0, 5 / edge=True
  minima_count (ws_kernels.hip), also through ws_segment_minima_device:
    al, w % 4 == 0, w >= 4                      k_minima_count<true>                  rows 7, 10; segment_minima aligned layouts
    not al, w % 4 == 0                          k_minima_count<false> (never run)     rows 2, 3, 6, 8, 9; segment_minima unaligned
    w % 4 != 0 or w < 4                         k_minima_count<false>                 rows 0, 5
  batch calls: stacked only for row_stride == w and slice_stride == h * row_stride (layout d, at an odd offset); layouts
    a, b, c take the slice loop with d_cube + k * slice_stride as base             test_cube_*
  graph key: same buffers with another row_stride must not replay                    test_graph_replay_*

ws_tile_block (the row-block descriptor of ws_segment_tiled_device) has no stride field -- its planes are "row stride w" by
definition -- so that call is covered with unaligned block bases; the stride of a tile is covered by ws_tile_block2d.img_stride.
"""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import oracle_lib as ol
import strided

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF)

# (h, w, field kind, offset, row stride): every w, h, offset class, stride kind and field kind of the issue occurs; rows 7-10
# add the aligned-but-strided and the unaligned-by-one-cause-only classes of the table above
PLANES = [
    (5, 3, "noise", 1, "w"),            # 0
    (31, 96, "smooth", 2, "w+1"),       # 1
    (70, 512, "noise", 3, "w+2"),       # 2
    (300, 520, "smooth", 0, "w+3"),     # 3
    (70, 772, "maze", 4, "w+4"),        # 4
    (31, 1030, "noise", 64, "pitch"),   # 5
    (70, 1056, "smooth", 1, "2w"),      # 6
    (70, 512, "noise", 0, "w+4"),       # 7
    (31, 96, "noise", 0, "w+2"),        # 8
    (70, 512, "smooth", 2, "w+4"),      # 9
    (300, 520, "noise", 64, "2w"),      # 10
]
IDS = [f"{i}-{h}x{w}-{k}-off{o}-{s}" for i, (h, w, k, o, s) in enumerate(PLANES)]


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def eng(pkg):
    import torch
    with torch.cuda.stream(torch.cuda.Stream(0)):      # a stream of its own: repeated transforms are captured and replayed
        yield importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


def _new_engine():
    return importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


@functools.lru_cache(maxsize=None)
def _case(h, w, kind):
    """(image, its seeds as a strictly increasing (n, 2) uint64 list)"""
    if kind == "maze":      # one winding corridor between walls: hundreds of rings, one seed at its end
        img = np.full((h, w), 255, np.uint8)
        for k, y in enumerate(range(2, h - 2, 4)):
            img[y, 2:w - 2] = 7
            img[y:y + 5, (w - 3) if k % 2 == 0 else 2] = 7
        img[h - 2:, :] = 255
        return img, np.array([[2, 2]], dtype=np.uint64)
    img = cases.field(h, w, 11 + h + w) if kind == "noise" else cases.smooth_field(h, w, 5 + h + w)
    seeds = np.asarray(ol.find_local_minima(img), dtype=np.uint64).reshape(-1, 2)
    if kind == "smooth" and len(seeds) > 3:      # few seeds: floods cross many tiles (long-range passes)
        seeds = seeds[:: max(len(seeds) // 3, 1)][:3]
    if len(seeds) == 0:
        seeds = np.array([[h // 2, w // 2]], dtype=np.uint64)
    return img, np.ascontiguousarray(seeds)


class Plane:
    """An image embedded in a larger device array."""

    def __init__(self, eng, img, offset, row_stride, fill):
        import torch
        self.host, self.off, self.mask = strided.embed(img, offset, row_stride, fill)
        self.t = torch.from_numpy(self.host).to(eng.device)
        assert self.t.data_ptr() % 256 == 0      # so that (pointer % 4) is (offset % 4), as the table above assumes
        self.ptr = self.t.data_ptr() + self.off
        self.h, self.w = img.shape
        self.rs = row_stride

    def unchanged(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.t.cpu().numpy() == self.host).all())


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and bool((a == b).all())
    return a == b


def _under_fills(eng, img, offset, row_stride, call):
    """call(plane) under both fills: identical results, the backing array untouched.  Returns the result."""
    res = []
    for fill in FILLS:
        p = Plane(eng, img, offset, row_stride, fill)
        res.append(call(p))
        assert p.unchanged(), ("the image is const", hex(fill))
    assert _same(res[0], res[1]), "the result depends on bytes outside the view"
    return res[0]


def _dev_seeds(eng, seeds):
    import torch
    s = np.asarray(seeds, dtype=np.int64).reshape(-1, 2).astype(np.int32)
    return torch.from_numpy(s).to(eng.device).contiguous()


def _opt(pkg, max_level=254, edge=False, engine=0, seed_shift=False):
    return pkg._ffi.Options(max_level, int(edge), engine, 0, int(seed_shift))


def _sync():
    import torch
    torch.cuda.synchronize()


# ---- the raw calls: always the library itself, with the plane's pointer and stride ---------------------------------------------------

def _minima(pkg, eng, ptr, h, w, rs, cap=None):
    import torch
    full = ((max(h, 1) - 1) // 2 + 1) * ((max(w, 1) - 1) // 2 + 1)
    cap = full if cap is None else cap
    out = torch.full((max(cap, 1), 2), -1, dtype=torch.int32, device=eng.device)
    n = ctypes.c_size_t(0)
    rc = pkg._ffi.lib().ws_find_local_minima_device(eng.ctx.handle, ptr, h, w, rs, out.data_ptr(), cap, ctypes.byref(n))
    _sync()
    return rc, n.value, out.cpu().numpy()


def _labels_buf(eng, h, w, edge, n=1):
    import torch
    e = 2 if edge else 0
    return torch.full((n, h + e, w + e), 0x5A5A5A5A, dtype=torch.int32, device=eng.device)


def _np32(t):
    _sync()
    return t.cpu().numpy().view(np.uint32)


def _segment(pkg, eng, ptr, h, w, rs, seeds, opt, fn="ws_segment_device"):
    d_seeds = _dev_seeds(eng, seeds)
    out = _labels_buf(eng, h, w, opt.edge_correction)
    rc = getattr(pkg._ffi.lib(), fn)(eng.ctx.handle, ptr, h, w, rs, d_seeds.data_ptr() if len(seeds) else None, len(seeds), ctypes.byref(opt),
                                     out.data_ptr())
    return rc, _np32(out)[0]


def _arrival(pkg, eng, ph, pw):
    import torch
    keys = torch.zeros((ph, pw), dtype=torch.int32, device=eng.device)
    assert pkg._ffi.lib().ws_copy_last_arrival_device(eng.ctx.handle, keys.data_ptr(), ph * pw) == 0
    return _np32(keys)


def _to_list(pkg, eng, ptr, h, w, rs, seeds, merging, opt):
    import torch
    levels = opt.max_water_level + 1
    cap = max(len(seeds), 1) * levels + 16      # (a level has at most one lake per seed)
    lakes = torch.zeros((cap, 2), dtype=torch.int64, device=eng.device)
    offsets = np.zeros(levels + 1, dtype=np.uint64)
    unc = np.zeros(levels, dtype=np.uint64)
    n = ctypes.c_size_t(0)
    d_seeds = _dev_seeds(eng, seeds)
    rc = pkg._ffi.lib().ws_transform_to_list_device(eng.ctx.handle, int(merging), ptr, h, w, rs, d_seeds.data_ptr() if len(seeds) else None, len(seeds),
                                                     ctypes.byref(opt), lakes.data_ptr(), cap, ctypes.byref(n), offsets.ctypes.data, unc.ctypes.data)
    _sync()
    return rc, _records(lakes[: n.value].cpu().numpy(), offsets, unc, 0, levels)


def _records(rec, offsets, unc, k, levels):
    """Slice k's lists in canonical form: per level (uncoloured, colours ascending, their areas) -- records as sets per level."""
    out = []
    for lvl in range(levels):
        b = k * levels + lvl
        r = rec[int(offsets[b]):int(offsets[b + 1])]
        o = np.argsort(r[:, 0], kind="stable")
        out.append((int(unc[b]), r[o, 0].astype(np.uint64), r[o, 1].astype(np.uint64)))
    return out


def _history(pkg, eng, ptr, h, w, rs, seeds, merging, opt, levels):
    import torch
    e = 2 if opt.edge_correction else 0
    n = (h + e) * (w + e)
    lv = np.asarray(levels, dtype=np.uint8)
    out = torch.full((len(levels), h + e, w + e), 0x5A5A5A5A, dtype=torch.int32, device=eng.device)
    d_seeds = _dev_seeds(eng, seeds)
    rc = pkg._ffi.lib().ws_transform_history_device(eng.ctx.handle, int(merging), ptr, h, w, rs, d_seeds.data_ptr() if len(seeds) else None, len(seeds),
                                                     ctypes.byref(opt), lv.ctypes.data, lv.size, out.data_ptr(), n)
    return rc, _np32(out)


# ---- the oracle on the COMPACT image --------------------------------------------------------------------------------------------------

def _oracle_lists(img, seeds, merging, max_level, edge=False):
    want = []

    def hook(l, m, i, c):
        hist = ol.find_lake_sizes(c)
        nz = np.nonzero(hist[1:])[0] + 1
        want.append((int(hist[0]), nz.astype(np.uint64), hist[nz].astype(np.uint64)))
    s = [tuple(map(int, p)) for p in seeds]
    if merging:
        ol.merge_arrival(img, s, max_level=max_level, edge=edge, hook=hook)      # canonical ids, as the engine's
    else:
        ol.segment(img, s, max_level=max_level, edge=edge, hook=hook)
    return want


def _oracle_levels(img, seeds, merging, levels, max_level=254, edge=False):
    snaps = []
    if merging:
        ol.merge(img, seeds, max_level=max_level, edge=edge, hook=lambda l, m, i, c: snaps.append(ol.canonicalise(c, seeds)[0]))
    else:
        ol.segment(img, seeds, max_level=max_level, edge=edge, hook=lambda l, m, i, c: snaps.append(c.copy()))
    return np.stack([snaps[l] for l in levels]).astype(np.uint32)


def _packed_keys(want_keys):
    """The oracle's stamps (level << 32 | ring, ~0 = never) in the engine's 32-bit form (level << 24 | ring, >= 0xFF000000 = never)."""
    never = want_keys == np.uint64(0xFFFFFFFFFFFFFFFF)
    return never, (((want_keys >> np.uint64(32)) << np.uint64(24)) | (want_keys & np.uint64(0xFFFFFF))).astype(np.uint32)


def _plane_args(i):
    h, w, kind, offset, sk = PLANES[i]
    img, seeds = _case(h, w, kind)
    return h, w, img, seeds, offset, strided.row_stride_of(sk, w)


# ---- 1. ws_find_local_minima_device -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(PLANES)), ids=IDS)
def test_find_local_minima_on_strided_planes(pkg, eng, i):
    h, w, img, _, offset, rs = _plane_args(i)
    want = np.asarray(ol.find_local_minima(img), dtype=np.int64).reshape(-1, 2)
    rc, n, out = _under_fills(eng, img, offset, rs, lambda p: _minima(pkg, eng, p.ptr, h, w, rs))
    assert rc == 0 and n == len(want) and (out[:n] == want).all()


@pytest.mark.parametrize("w", [3, 96, 512, 520, 772, 1030, 1056])
def test_find_local_minima_every_width_against_every_offset(pkg, eng, w):
    # the dispatcher's test is (pointer | stride) % 4 with w % 4: every offset class with a stride of either class, h = 31
    img = cases.field(31, w, 900 + w)
    want = np.asarray(ol.find_local_minima(img), dtype=np.int64).reshape(-1, 2)
    for offset, sk in ((0, "w+4"), (1, "w"), (2, "w+2"), (3, "pitch"), (4, "w+1"), (64, "2w"), (0, "w+3")):
        rs = strided.row_stride_of(sk, w)
        rc, n, out = _under_fills(eng, img, offset, rs, lambda p: _minima(pkg, eng, p.ptr, 31, w, rs))
        assert rc == 0 and n == len(want) and (out[:n] == want).all(), (offset, sk)


def test_find_local_minima_capacity_protocol_on_a_strided_plane(pkg, eng):
    h, w = 70, 512
    img = cases.field(h, w, 77)
    want = np.asarray(ol.find_local_minima(img), dtype=np.int64).reshape(-1, 2)
    cap = len(want) // 2

    def call(p):
        rc, n, out = _minima(pkg, eng, p.ptr, h, w, p.rs, cap=cap)
        rc2, n2, out2 = _minima(pkg, eng, p.ptr, h, w, p.rs, cap=n)      # call again with the count reported
        return rc, n, out, rc2, n2, out2
    rc, n, out, rc2, n2, out2 = _under_fills(eng, img, 3, w + 1, call)
    assert rc == pkg._ffi.WS_ERR_CAPACITY and n == len(want)              # *n_found still holds the true count
    assert (out[:cap] == want[:cap]).all()
    assert rc2 == 0 and n2 == len(want) and (out2[:n2] == want).all()


# ---- 2. ws_segment_device ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("engine_name", ["ENGINE_FUSED", "ENGINE_SWEEP"])
@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("i", range(len(PLANES)), ids=IDS)
def test_segment_table_form(pkg, eng, i, edge, engine_name):
    h, w, img, seeds, offset, rs = _plane_args(i)
    opt = _opt(pkg, 254, edge, getattr(pkg, engine_name))
    rc, got = _under_fills(eng, img, offset, rs, lambda p: _segment(pkg, eng, p.ptr, h, w, rs, seeds, opt))
    want = ol.segment_arrival(img, seeds, edge=edge)
    assert rc == 0 and got.shape == want.shape and (got == want).all(), int((got != want).sum())


@pytest.mark.parametrize("i", range(len(PLANES)), ids=IDS)
def test_segment_painted_form_low_level_seed_shift_and_arrival_stamps(pkg, eng, i):
    h, w, img, seeds, offset, rs = _plane_args(i)
    rng = np.random.default_rng(5 + i)
    if PLANES[i][2] == "noise" and len(seeds) > 4:
        base = seeds
    else:      # more seeds than the case's few, so that there is something to shuffle
        base = np.asarray(ol.find_local_minima(img), dtype=np.uint64).reshape(-1, 2)
        base = base if len(base) > 1 else np.concatenate([seeds, seeds])
    shuffled = np.ascontiguousarray(np.concatenate([base, base[::3]])[rng.permutation(len(base) + len(base[::3]))])
    fused = pkg.ENGINE_FUSED

    def call(p):
        res = []
        # a shuffled list with duplicates: the painted (label-plane) form; the later entry wins
        res.append(_segment(pkg, eng, p.ptr, h, w, rs, shuffled, _opt(pkg, 254, False, fused)))
        res.append(_arrival(pkg, eng, h, w))
        # a low water level, both seed forms
        res.append(_segment(pkg, eng, p.ptr, h, w, rs, seeds, _opt(pkg, 40, False, fused)))
        res.append(_segment(pkg, eng, p.ptr, h, w, rs, shuffled, _opt(pkg, 40, True, fused)))
        # edge correction with the seeds moved onto their own pixels
        res.append(_segment(pkg, eng, p.ptr, h, w, rs, seeds, _opt(pkg, 254, True, fused, seed_shift=True)))
        # the table form's stamps
        res.append(_segment(pkg, eng, p.ptr, h, w, rs, seeds, _opt(pkg, 254, False, fused)))
        res.append(_arrival(pkg, eng, h, w))
        return res
    (rc0, painted), keys0, (rc1, low), (rc2, low_edge), (rc3, shifted), (rc4, table), keys1 = _under_fills(eng, img, offset, rs, call)
    assert rc0 == rc1 == rc2 == rc3 == rc4 == 0
    want, wkeys = ol.segment_arrival(img, shuffled, want_keys=True)
    assert (painted == want).all()
    never, packed = _packed_keys(wkeys)
    assert (keys0[~never] == packed[~never]).all() and (keys0[never] >= 0xFF000000).all()
    assert (low == ol.segment_arrival(img, seeds, max_level=40)).all()
    assert (low_edge == ol.segment_arrival(img, shuffled, max_level=40, edge=True)).all()
    assert (shifted == ol.segment_arrival(img, seeds + 1, edge=True)).all()
    want, wkeys = ol.segment_arrival(img, seeds, want_keys=True)
    never, packed = _packed_keys(wkeys)
    assert (table == want).all()
    assert (keys1[~never] == packed[~never]).all() and (keys1[never] >= 0xFF000000).all()


# ---- 3. ws_segment_minima_device --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("h,w,kind,offset,sk", [
    (70, 512, "noise", 0, "w+4"), (70, 512, "noise", 3, "w+1"),        # w % 32 == 0: the fused form (tables out of the minima kernels)
    (31, 96, "smooth", 64, "pitch"), (70, 1056, "noise", 2, "2w"),
    (300, 520, "noise", 4, "w+4"), (300, 520, "smooth", 1, "w+3"),     # w % 32 != 0: the internal pair
    (70, 772, "noise", 0, "pitch"), (31, 1030, "noise", 2, "w+2"), (5, 3, "noise", 1, "w")])
def test_segment_minima_is_the_call_pair_on_the_compact_image(pkg, eng, h, w, kind, offset, sk, edge):
    import torch
    img = cases.field(h, w, 400 + w) if kind == "noise" else cases.smooth_field(h, w, 400 + w)
    rs = strided.row_stride_of(sk, w)
    seeds = np.asarray(ol.find_local_minima(img), dtype=np.uint64).reshape(-1, 2)
    want = ol.segment_arrival(img, seeds, edge=edge)
    opt = _opt(pkg, 254, edge, pkg.ENGINE_FUSED)
    cap = ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1)

    def call(p):
        out = _labels_buf(eng, h, w, edge)
        lst = torch.full((cap, 2), -1, dtype=torch.int32, device=eng.device)
        n = ctypes.c_size_t(0)
        rc = pkg._ffi.lib().ws_segment_minima_device(eng.ctx.handle, p.ptr, h, w, rs, ctypes.byref(opt), out.data_ptr(), lst.data_ptr(), cap, ctypes.byref(n))
        out2 = _labels_buf(eng, h, w, edge)
        n2 = ctypes.c_size_t(0)      # ... and without the list
        rc2 = pkg._ffi.lib().ws_segment_minima_device(eng.ctx.handle, p.ptr, h, w, rs, ctypes.byref(opt), out2.data_ptr(), None, 0, ctypes.byref(n2))
        return rc, n.value, _np32(out)[0], _np32(lst), rc2, n2.value, _np32(out2)[0]
    rc, n, got, lst, rc2, n2, got2 = _under_fills(eng, img, offset, rs, call)
    assert rc == rc2 == 0 and n == n2 == len(seeds)
    assert (lst[:n] == seeds.astype(np.uint32)).all()
    assert (got == want).all() and (got2 == want).all()


# ---- 4. ws_merge_device -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edge,max_level", [(False, 254), (True, 120)])
@pytest.mark.parametrize("i", range(len(PLANES)), ids=IDS)
def test_merge_final_labels(pkg, eng, i, edge, max_level):
    h, w, img, _, offset, rs = _plane_args(i)
    seeds = _case(h, w, PLANES[i][2])[1] if PLANES[i][2] == "maze" else np.asarray(ol.find_local_minima(img), dtype=np.uint64).reshape(-1, 2)
    if len(seeds) == 0:
        seeds = _case(h, w, PLANES[i][2])[1]
    opt = _opt(pkg, max_level, edge)
    rc, got = _under_fills(eng, img, offset, rs, lambda p: _segment(pkg, eng, p.ptr, h, w, rs, seeds, opt, fn="ws_merge_device"))
    assert rc == 0 and (got == ol.merge_arrival(img, seeds, max_level=max_level, edge=edge)).all()


# ---- 5. ws_transform_to_list_device -----------------------------------------------------------------------------------------------------

def _lists_equal(got, want):
    assert len(got) == len(want)
    for lvl, ((gu, gc, ga), (wu, wc, wa)) in enumerate(zip(got, want)):
        assert gu == wu and gc.shape == wc.shape and (gc == wc).all() and (ga == wa).all(), lvl


@pytest.mark.parametrize("merging", [True, False])
@pytest.mark.parametrize("i", range(len(PLANES)), ids=IDS)
def test_transform_to_list(pkg, eng, i, merging):
    h, w, img, seeds, offset, rs = _plane_args(i)
    if PLANES[i][2] == "noise":
        seeds = seeds[:: 3]      # still strictly increasing; fewer records
    max_level = 254 if h * w < 60000 else 90
    edge = i % 2 == 1
    opt = _opt(pkg, max_level, edge)
    rc, got = _under_fills(eng, img, offset, rs, lambda p: _to_list(pkg, eng, p.ptr, h, w, rs, seeds, merging, opt))
    assert rc == 0
    _lists_equal(got, _oracle_lists(img, seeds, merging, max_level, edge))


# ---- 6. ws_transform_history_device -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("merging", [True, False])
@pytest.mark.parametrize("i", range(len(PLANES)), ids=IDS)
def test_transform_history(pkg, eng, i, merging):
    h, w, img, seeds, offset, rs = _plane_args(i)
    if PLANES[i][2] == "noise":
        seeds = seeds[:: 2]
    edge = i % 2 == 0
    levels = [200, 0, 37, 254, 37, 120]
    opt = _opt(pkg, 254, edge)
    rc, got = _under_fills(eng, img, offset, rs, lambda p: _history(pkg, eng, p.ptr, h, w, rs, seeds, merging, opt, levels))
    want = _oracle_levels(img, seeds, merging, levels, edge=edge)
    assert rc == 0 and got.shape == want.shape and (got == want).all()


# ---- 7. schedules picked by context switches ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,kind,offset,sk", [
    (70, 512, "noise", 1, "w+3"), (70, 512, "noise", 0, "w+4"),
    (300, 520, "smooth", 3, "pitch"), (300, 520, "smooth", 64, "2w"),
    (70, 772, "noise", 2, "w"), (70, 772, "noise", 4, "pitch")])
def test_seam_repair_on_strided_planes(pkg, h, w, kind, offset, sk):
    import torch
    img = cases.field(h, w, 77) if kind == "noise" else cases.smooth_field(h, w, 41)
    seeds = np.asarray(ol.find_local_minima(img), dtype=np.uint64).reshape(-1, 2)
    rs = strided.row_stride_of(sk, w)
    with torch.cuda.stream(torch.cuda.Stream(0)):
        e = _new_engine()
        e.ctx.set_seam_repair_min_pixels(1)
        stats = []

        def call(p):
            res = []
            for _ in range(2):      # the second call replays a captured graph
                res.append(_segment(pkg, e, p.ptr, h, w, rs, seeds, _opt(pkg, 254, False, pkg.ENGINE_FUSED)))
                stats.append(e.ctx.stats())
            res.append(_segment(pkg, e, p.ptr, h, w, rs, seeds, _opt(pkg, 100, False, pkg.ENGINE_FUSED)))
            res.append(_segment(pkg, e, p.ptr, h, w, rs, seeds, _opt(pkg, 254), fn="ws_merge_device"))
            return res
        (rc0, a), (rc1, b), (rc2, lo), (rc3, mg) = _under_fills(e, img, offset, rs, call)
        e.ctx.set_seam_repair_min_pixels(0)
    assert rc0 == rc1 == rc2 == rc3 == 0
    want = ol.segment_arrival(img, seeds)
    assert (a == want).all() and (b == want).all()
    for st in stats:
        assert st["launches_relax"] == st["relax_passes"] + 1      # pass 1 was two launches (bands, strips): the seam flow ran
    assert (lo == ol.segment_arrival(img, seeds, max_level=100)).all()
    assert (mg == ol.merge_arrival(img, seeds)).all()


@pytest.mark.parametrize("mode", [1, 2, 4])
@pytest.mark.parametrize("offset,sk", [(3, "w+2"), (0, "w+4"), (2, "pitch"), (64, "2w")])
def test_persistent_pass_modes_on_strided_planes(pkg, mode, offset, sk):
    import torch
    h, w = 300, 520
    img = cases.smooth_field(h, w, 23, octaves=5)
    seeds = np.asarray(ol.find_local_minima(img), dtype=np.uint64).reshape(-1, 2)
    seeds = np.ascontiguousarray(seeds[:: max(len(seeds) // 3, 1)][:3])
    rs = strided.row_stride_of(sk, w)
    set_mode = pkg._ffi.lib().ws_ctx_set_persistent_pass
    with torch.cuda.stream(torch.cuda.Stream(0)):
        e = _new_engine()
        assert set_mode(e.ctx.handle, mode) == 0
        stats = []

        def call(p):
            r = _segment(pkg, e, p.ptr, h, w, rs, seeds, _opt(pkg, 254, False, pkg.ENGINE_FUSED))
            stats.append(e.ctx.stats()["relax_passes"])
            return r
        rc, got = _under_fills(e, img, offset, rs, call)
        assert set_mode(e.ctx.handle, 3) == 0
    assert rc == 0 and (got == ol.segment_arrival(img, seeds)).all()
    assert min(stats) >= 5      # the flood got as far as the late passes (mode 2: the queue is pass 3, pass 4 looks at every tile again)


# ---- 8. graph replay ----------------------------------------------------------------------------------------------------------------------

def _rewrite(t, img, offset, row_stride, fill):
    """The backing tensor rewritten so that the view (offset, row_stride) is `img`; everything else `fill`."""
    import torch
    host, off, _ = strided.embed(img, offset, row_stride, fill)
    full = np.full(t.numel(), fill, dtype=np.uint8)
    full[: host.size] = host
    t.copy_(torch.from_numpy(full))
    return full


@pytest.mark.parametrize("form", ["segment", "segment_begin_end", "merge", "merge_begin_end"])
@pytest.mark.parametrize("offset,sk,sk2", [(3, "w+1", "w+3"), (0, "w+4", "2w")])
def test_graph_replay_on_strided_planes_and_a_change_of_stride(pkg, form, offset, sk, sk2):
    import torch
    L = pkg._ffi.lib()
    h, w = 96, 256
    imgs = [cases.field(h, w, 500), cases.smooth_field(h, w, 501), cases.field(h, w, 502), cases.field(h, w, 503)]
    lists = [np.asarray(ol.find_local_minima(a), dtype=np.uint64).reshape(-1, 2) for a in imgs]
    n = min(len(x) for x in lists)
    rs, rs2 = strided.row_stride_of(sk, w), strided.row_stride_of(sk2, w)
    merging = form.startswith("merge")
    oracle = ol.merge_arrival if merging else ol.segment_arrival
    with torch.cuda.stream(torch.cuda.Stream(0)):      # capture is not allowed on the legacy null stream
        e = _new_engine()
        t = torch.zeros(strided.plane_bytes(h, w, offset, max(rs, rs2)), dtype=torch.uint8, device=e.device)
        ptr = t.data_ptr() + strided.GUARD + offset
        d_seeds = torch.empty((n, 2), dtype=torch.int32, device=e.device)
        out = torch.empty((h, w), dtype=torch.int32, device=e.device)
        opt = _opt(pkg, 254)

        def run(stride):
            args = (e.ctx.handle, ptr, h, w, stride, d_seeds.data_ptr(), n, ctypes.byref(opt), out.data_ptr())
            if form == "segment":
                rc = L.ws_segment_device(*args)
            elif form == "merge":
                rc = L.ws_merge_device(*args)
            elif form == "segment_begin_end":
                rc = L.ws_segment_device_begin(*args) or L.ws_segment_device_end(e.ctx.handle)
            else:
                rc = L.ws_merge_device_begin(*args) or L.ws_merge_device_end(e.ctx.handle)
            assert rc == 0, (rc, L.ws_last_error(e.ctx.handle))
            return _np32(out).copy()

        for rep in range(3):      # the same strided call, the CONTENTS rewritten in between
            fill = FILLS[rep % 2]
            host = _rewrite(t, imgs[rep], offset, rs, fill)
            d_seeds.copy_(torch.from_numpy(lists[rep][:n].astype(np.int32)))
            got = run(rs)
            assert (got == oracle(imgs[rep], lists[rep][:n])).all(), rep
            assert (t.cpu().numpy() == host).all()
        assert e.ctx.stats()["graph_launches"] == 1      # captured by the second call, replayed by the third
        # the same base pointer, sizes, seed and label buffers with ANOTHER row_stride: the new view is another image
        host = _rewrite(t, imgs[3], offset, rs2, 0x00)
        d_seeds.copy_(torch.from_numpy(lists[3][:n].astype(np.int32)))
        got = run(rs2)
        assert e.ctx.stats()["graph_launches"] == 0      # another key: nothing of the old launches is replayed
        assert (got == oracle(imgs[3], lists[3][:n])).all()
        host = _rewrite(t, imgs[3], offset, rs2, 0xFF)
        assert (run(rs2) == got).all()
        assert (t.cpu().numpy() == host).all()
        # ... and back: the first stride again on the same buffers
        _rewrite(t, imgs[1], offset, rs, 0x00)
        d_seeds.copy_(torch.from_numpy(lists[1][:n].astype(np.int32)))
        assert (run(rs) == oracle(imgs[1], lists[1][:n])).all()


# ---- 9. cubes -----------------------------------------------------------------------------------------------------------------------------

class Cube:
    def __init__(self, eng, cube, offset, row_stride, slice_stride, fill):
        import torch
        self.host, self.off, self.mask = strided.embed_cube(cube, offset, row_stride, slice_stride, fill)
        self.t = torch.from_numpy(self.host).to(eng.device)
        assert self.t.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr() + self.off

    def unchanged(self):
        _sync()
        return bool((self.t.cpu().numpy() == self.host).all())


def _cube_layouts(h, w):
    """name -> (offset, row_stride, slice_stride): the issue's (a) to (d)"""
    return {"a_rows": (0, w + 4, h * (w + 4)), "a_rows_unaligned": (1, w + 3, h * (w + 3)),
            "b_gap_1_byte": (2, w, h * w + 1), "b_gap_one_row": (4, w, h * w + w),
            "c_both": (3, w + 5, h * (w + 5) + 7), "c_both_aligned": (64, 2 * w, h * 2 * w + 256),
            "d_contiguous_odd_offset": (1, w, h * w), "d_contiguous_offset_2": (2, w, h * w)}


def _cube_case(s, h, w, first_seed):
    imgs = [cases.field(h, w, first_seed + 7 * k) if k % 2 == 0 else cases.smooth_field(h, w, first_seed + 7 * k) for k in range(s)]
    lists = [np.asarray(ol.find_local_minima(im), dtype=np.uint64).reshape(-1, 2) for im in imgs]
    assert all(len(l) for l in lists)
    offs = [0] + [int(x) for x in np.cumsum([len(l) for l in lists])]
    return np.stack(imgs), lists, offs


def _c_offsets(offs):
    return (ctypes.c_size_t * len(offs))(*offs)


def _under_fills_cube(eng, cube, layout, call):
    res = []
    for fill in FILLS:
        c = Cube(eng, cube, layout[0], layout[1], layout[2], fill)
        res.append(call(c))
        assert c.unchanged(), ("the cube is const", hex(fill))
    assert _same(res[0], res[1]), "the result depends on bytes outside the slices"
    return res[0]


def _last_arrival_status(pkg, eng):
    p, hh, ww = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
    return pkg._ffi.lib().ws_last_arrival_device(eng.ctx.handle, ctypes.byref(p), ctypes.byref(hh), ctypes.byref(ww))


CUBE_SHAPES = [(5, 32, 96, False), (4, 30, 94, True), (3, 64, 128, False)]      # the (padded) plane: w' % 4 == 0, h' * w' % 128 == 0 -- a contiguous cube stacks


@pytest.mark.parametrize("s,h,w,edge", CUBE_SHAPES)
def test_cube_segment_batch(pkg, s, h, w, edge):
    e = _new_engine()
    cube, lists, offs = _cube_case(s, h, w, 1000)
    d_seeds = _dev_seeds(e, np.concatenate(lists))
    opt = _opt(pkg, 254, edge)
    want = [ol.segment_arrival(cube[k], lists[k], edge=edge) for k in range(s)]
    for name, (offset, rs, ss) in _cube_layouts(h, w).items():
        def call(c):
            out = _labels_buf(e, h, w, edge, s)
            failed = ctypes.c_size_t(99)
            rc = pkg._ffi.lib().ws_segment_batch_device(e.ctx.handle, c.ptr, s, h, w, rs, ss, d_seeds.data_ptr(), _c_offsets(offs), ctypes.byref(opt),
                                                         out.data_ptr(), ctypes.byref(failed))
            return rc, failed.value, _np32(out), _last_arrival_status(pkg, e)
        rc, failed, got, arrival = _under_fills_cube(e, cube, (offset, rs, ss), call)
        assert rc == 0 and failed == 0, name
        for k in range(s):
            assert (got[k] == want[k]).all(), (name, k)
        # a stacked batch leaves no slice's stamps behind; the loop leaves the last slice's
        assert arrival == (pkg._ffi.WS_ERR_UNSUPPORTED if name.startswith("d_") else 0), name


@pytest.mark.parametrize("s,h,w,edge", CUBE_SHAPES)
def test_cube_merge_batch(pkg, s, h, w, edge):
    e = _new_engine()
    cube, lists, offs = _cube_case(s, h, w, 1100)
    d_seeds = _dev_seeds(e, np.concatenate(lists))
    opt = _opt(pkg, 120, edge)
    want = [ol.merge_arrival(cube[k], lists[k], max_level=120, edge=edge) for k in range(s)]
    passes = {}
    for name, (offset, rs, ss) in list(_cube_layouts(h, w).items()) + [("control_compact", (0, w, h * w))]:
        def call(c):
            out = _labels_buf(e, h, w, edge, s)
            failed = ctypes.c_size_t(99)
            rc = pkg._ffi.lib().ws_merge_batch_device(e.ctx.handle, c.ptr, s, h, w, rs, ss, d_seeds.data_ptr(), _c_offsets(offs), ctypes.byref(opt),
                                                       out.data_ptr(), ctypes.byref(failed))
            passes[name] = e.ctx.stats()["relax_passes"]
            return rc, failed.value, _np32(out)
        rc, failed, got = _under_fills_cube(e, cube, (offset, rs, ss), call)
        assert rc == 0 and failed == 0, name
        for k in range(s):
            assert (got[k] == want[k]).all(), (name, k)
    _assert_stack_or_loop(passes, s)


def _assert_stack_or_loop(passes, s):
    """The statistics of a batch are summed over its transforms, and every transform runs at least two relaxation passes (pass 0
    and the pass that finds nothing left to do).  The loop over s slices therefore reports at least 2 s passes and more than the
    stack, which is ONE transform over all slices; layout (d) must report what the compact, aligned control reports, which the
    existing batch tests show to stack."""
    stack = passes["control_compact"]
    for name, p in passes.items():
        if name.startswith("d_"):
            assert p == stack, (name, passes)
        elif name != "control_compact":
            assert p >= 2 * s and p > stack, (name, passes)


@pytest.mark.parametrize("merging", [True, False])
@pytest.mark.parametrize("s,h,w,edge", CUBE_SHAPES)
def test_cube_transform_to_list_batch(pkg, s, h, w, edge, merging):
    import torch
    e = _new_engine()
    cube, lists, offs = _cube_case(s, h, w, 1200)
    lists = [l[::2] for l in lists]
    offs = [0] + [int(x) for x in np.cumsum([len(l) for l in lists])]
    d_seeds = _dev_seeds(e, np.concatenate(lists))
    max_level = 90
    levels = max_level + 1
    opt = _opt(pkg, max_level, edge)
    want = [_oracle_lists(cube[k], lists[k], merging, max_level, edge) for k in range(s)]
    cap = offs[-1] * levels + 16
    passes = {}
    for name, (offset, rs, ss) in list(_cube_layouts(h, w).items()) + [("control_compact", (0, w, h * w))]:
        def call(c):
            lakes = torch.zeros((cap, 2), dtype=torch.int64, device=e.device)
            offsets = np.zeros(s * levels + 1, dtype=np.uint64)
            unc = np.zeros(s * levels, dtype=np.uint64)
            n, failed = ctypes.c_size_t(0), ctypes.c_size_t(99)
            rc = pkg._ffi.lib().ws_transform_to_list_batch_device(e.ctx.handle, int(merging), c.ptr, s, h, w, rs, ss, d_seeds.data_ptr(), _c_offsets(offs),
                                                                   ctypes.byref(opt), lakes.data_ptr(), cap, ctypes.byref(n), offsets.ctypes.data,
                                                                   unc.ctypes.data, ctypes.byref(failed))
            _sync()
            passes[name] = e.ctx.stats()["relax_passes"]
            rec = lakes[: n.value].cpu().numpy()
            return rc, failed.value, [_records(rec, offsets, unc, k, levels) for k in range(s)]
        rc, failed, got = _under_fills_cube(e, cube, (offset, rs, ss), call)
        assert rc == 0 and failed == 0, name
        for k in range(s):
            _lists_equal(got[k], want[k])
    _assert_stack_or_loop(passes, s)


@pytest.mark.parametrize("merging", [True, False])
@pytest.mark.parametrize("s,h,w,edge", CUBE_SHAPES)
def test_cube_transform_history_batch(pkg, s, h, w, edge, merging):
    import torch
    e = _new_engine()
    cube, lists, offs = _cube_case(s, h, w, 1300)
    d_seeds = _dev_seeds(e, np.concatenate(lists))
    levels = [254, 0, 60, 131]
    lv = np.asarray(levels, dtype=np.uint8)
    opt = _opt(pkg, 254, edge)
    x = 2 if edge else 0
    plane = (h + x) * (w + x)
    want = [_oracle_levels(cube[k], lists[k], merging, levels, edge=edge) for k in range(s)]
    passes = {}
    for name, (offset, rs, ss) in list(_cube_layouts(h, w).items()) + [("control_compact", (0, w, h * w))]:
        def call(c):
            out = torch.full((s, len(levels), h + x, w + x), 0x5A5A5A5A, dtype=torch.int32, device=e.device)
            failed = ctypes.c_size_t(99)
            rc = pkg._ffi.lib().ws_transform_history_batch_device(e.ctx.handle, int(merging), c.ptr, s, h, w, rs, ss, d_seeds.data_ptr(), _c_offsets(offs),
                                                                   ctypes.byref(opt), lv.ctypes.data, lv.size, out.data_ptr(), plane, ctypes.byref(failed))
            passes[name] = e.ctx.stats()["relax_passes"]
            return rc, failed.value, _np32(out)
        rc, failed, got = _under_fills_cube(e, cube, (offset, rs, ss), call)
        assert rc == 0 and failed == 0, name
        for k in range(s):
            assert (got[k] == want[k]).all(), (name, k)
    _assert_stack_or_loop(passes, s)


def test_cube_with_a_failing_slice_names_it(pkg):
    import torch
    e = _new_engine()
    s, h, w = 4, 32, 96
    cube, lists, _ = _cube_case(s, h, w, 1400)
    lists[2] = np.concatenate([lists[2], np.array([[h, 5]], dtype=np.uint64)])      # a seed below its own slice
    offs = [0] + [int(x) for x in np.cumsum([len(l) for l in lists])]
    d_seeds = _dev_seeds(e, np.concatenate(lists))
    opt = _opt(pkg, 254)
    L = pkg._ffi.lib()
    offset, rs, ss = _cube_layouts(h, w)["c_both"]
    lv = np.asarray([0, 254], dtype=np.uint8)

    def call(c):
        res = []
        out = _labels_buf(e, h, w, False, s)
        failed = ctypes.c_size_t(99)
        res.append((L.ws_segment_batch_device(e.ctx.handle, c.ptr, s, h, w, rs, ss, d_seeds.data_ptr(), _c_offsets(offs), ctypes.byref(opt), out.data_ptr(),
                                              ctypes.byref(failed)), failed.value, _np32(out)[:2].copy()))
        failed = ctypes.c_size_t(99)
        res.append((L.ws_merge_batch_device(e.ctx.handle, c.ptr, s, h, w, rs, ss, d_seeds.data_ptr(), _c_offsets(offs), ctypes.byref(opt), out.data_ptr(),
                                            ctypes.byref(failed)), failed.value))
        lakes = torch.zeros((offs[-1] * 255 + 16, 2), dtype=torch.int64, device=e.device)
        o, u, n = np.zeros(s * 255 + 1, dtype=np.uint64), np.zeros(s * 255, dtype=np.uint64), ctypes.c_size_t(0)
        failed = ctypes.c_size_t(99)
        res.append((L.ws_transform_to_list_batch_device(e.ctx.handle, 1, c.ptr, s, h, w, rs, ss, d_seeds.data_ptr(), _c_offsets(offs), ctypes.byref(opt),
                                                        lakes.data_ptr(), lakes.shape[0], ctypes.byref(n), o.ctypes.data, u.ctypes.data, ctypes.byref(failed)),
                    failed.value))
        hist = torch.zeros((s, 2, h, w), dtype=torch.int32, device=e.device)
        failed = ctypes.c_size_t(99)
        res.append((L.ws_transform_history_batch_device(e.ctx.handle, 0, c.ptr, s, h, w, rs, ss, d_seeds.data_ptr(), _c_offsets(offs), ctypes.byref(opt),
                                                        lv.ctypes.data, 2, hist.data_ptr(), h * w, ctypes.byref(failed)), failed.value))
        _sync()
        return res
    seg, mer, lst, his = _under_fills_cube(e, cube, (offset, rs, ss), call)
    oob = pkg._ffi.WS_ERR_SEED_OOB
    assert seg[0] == oob and seg[1] == 2
    for k in range(2):      # the slices before the failing one are complete
        assert (seg[2][k] == ol.segment_arrival(cube[k], lists[k])).all(), k
    assert mer == (oob, 2) and lst == (oob, 2) and his == (oob, 2)


# ---- 10. row blocks and tiles ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,kind,offset,sk", [(70, 512, "noise", 0, "w+4"), (70, 512, "smooth", 3, "w+1"), (300, 520, "noise", 2, "pitch")])
def test_block_begin_relax_halo_resolve_local_on_a_strided_block(pkg, h, w, kind, offset, sk):
    # one block that is the whole field: no neighbour, so its local resolve is the transform's answer
    import torch
    e = _new_engine()
    L = pkg._ffi.lib()
    img, seeds = _case(h, w, kind)
    rs = strided.row_stride_of(sk, w)
    d_seeds = _dev_seeds(e, seeds)

    def call(p):
        keys = torch.zeros((h, w), dtype=torch.int32, device=e.device)
        lab = _labels_buf(e, h, w, False)
        rc = [L.ws_block_begin(e.ctx.handle, p.ptr, h, w, rs, 254, d_seeds.data_ptr(), len(seeds), 1, keys.data_ptr())]
        before = _np32(keys).copy()
        # the halo repair on a converged plane: it loads the border tiles' image rows again and must find nothing to change
        rc.append(L.ws_block_relax_halo(e.ctx.handle, p.ptr, h, w, rs, 254, 1, 1, keys.data_ptr()))
        after = _np32(keys).copy()
        rc.append(L.ws_block_resolve_local(e.ctx.handle, keys.data_ptr(), lab.data_ptr(), h, w, 0, 0))
        return rc, before, after, _np32(lab)[0]
    rc, before, after, got = _under_fills(e, img, offset, rs, call)
    assert rc == [0, 0, 0]
    want, wkeys = ol.segment_arrival(img, seeds, want_keys=True)
    never, packed = _packed_keys(wkeys)
    for keys in (before, after):
        assert (keys[~never] == packed[~never]).all() and (keys[never] >= 0xFF000000).all()
    assert (got == want).all()


@pytest.mark.parametrize("merging", [False, True])
@pytest.mark.parametrize("offset", [1, 2, 64])
def test_tiled_row_blocks_at_unaligned_bases(pkg, offset, merging):
    # ws_tile_block has no stride (row stride w by definition): two local ranks whose planes start at unaligned addresses
    import torch
    grp = importlib.import_module("rustronomy_watershed_amd.group").Group.local(2)
    ffi, L = pkg._ffi, pkg._ffi.lib()
    H, W = 140, 520
    img = cases.smooth_field(H, W, 61)
    seeds = np.asarray(ol.find_local_minima(img), dtype=np.uint64).reshape(-1, 2)
    want = (ol.merge_arrival if merging else ol.segment_arrival)(img, seeds, max_level=200)
    dev = torch.device("cuda", 0)
    results = []
    for fill in FILLS:
        blocks = (ffi.TileBlock * 2)()
        keep, spans = [], []
        for r in range(2):
            v = [ctypes.c_size_t() for _ in range(4)]
            assert L.ws_tile_rows(H, r, 2, *[ctypes.byref(x) for x in v]) == 0
            r0, r1, lo, hi = (x.value for x in v)
            host, off, _ = strided.embed(img[lo:hi], offset + r, W, fill)
            t = torch.from_numpy(host).to(dev)
            mine = (seeds[:, 0] >= lo) & (seeds[:, 0] < hi)
            i0 = int(np.argmax(mine)) if mine.any() else 0
            loc = seeds[mine].astype(np.int64)
            loc[:, 0] -= lo
            d_loc = torch.from_numpy(loc.astype(np.int32)).to(dev).contiguous()
            lab = torch.full((hi - lo, W), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            keep += [t, d_loc, lab]
            spans.append((r0, r1, lo, lab, t, host))
            blocks[r] = ffi.TileBlock(t.data_ptr() + off, d_loc.data_ptr() if len(loc) else None, None, len(loc), i0 + 1, 0, lab.data_ptr())
        _sync()
        opt = ffi.Options(200)
        rounds = ctypes.c_uint32(0)
        rc = L.ws_segment_tiled_device(grp._h, H, W, len(seeds), blocks, ctypes.byref(opt), int(merging), ctypes.byref(rounds))
        assert rc == 0, (rc, L.ws_group_last_error(grp._h))
        _sync()
        got = np.zeros((H, W), dtype=np.uint32)
        for r0, r1, lo, lab, t, host in spans:
            got[r0:r1] = lab.cpu().numpy().view(np.uint32)[r0 - lo:r1 - lo]
            assert (t.cpu().numpy() == host).all()
        results.append(got)
    grp.close()
    assert (results[0] == want).all() and (results[1] == want).all()


@pytest.mark.parametrize("offset,sk", [(3, "w+5"), (0, "pitch")])
def test_tiles_2d_as_views_into_a_wider_field(pkg, offset, sk):
    # ws_tile_block2d.img_stride: every tile a view into the embedded field, whose own row stride exceeds its width
    import torch
    grp_mod = importlib.import_module("rustronomy_watershed_amd.group")
    H, W, py, px = 120, 300, 1, 2
    img = cases.smooth_field(H, W, 71)
    seeds = np.asarray(ol.find_local_minima(img), dtype=np.uint64).reshape(-1, 2)
    want = ol.segment_arrival(img, seeds)
    rs = W + 5 if sk == "w+5" else strided.row_stride_of(sk, W)
    dev = torch.device("cuda", 0)
    results = []
    for fill in FILLS:
        g = grp_mod.Group.local(py * px)
        host, off, _ = strided.embed(img, offset, rs, fill)
        t = torch.from_numpy(host).to(dev)
        field = torch.as_strided(t, (H, W), (rs, 1), off)
        s = torch.from_numpy(seeds.astype(np.int64).astype(np.int32)).to(dev)
        blocks, spans, keep = g.make_blocks2d(field, s, py, px)
        for i in range(py * px):
            assert blocks[i].img_stride == rs and blocks[i].img_stride > spans[i][1][3] - spans[i][1][2]
        g.segment_tiled2d_device(H, W, py, px, blocks, n_seeds_total=len(seeds))
        _sync()
        got = np.zeros((H, W), dtype=np.uint32)
        for (r0, r1, lo, hi), (c0, c1, clo, chi), lab in spans:
            got[r0:r1, c0:c1] = lab.cpu().numpy().view(np.uint32)[r0 - lo:r1 - lo, c0 - clo:c1 - clo]
        assert (t.cpu().numpy() == host).all()
        g.close()
        results.append(got)
    assert (results[0] == want).all() and (results[1] == want).all()


# ---- 11. ws_random_field_device -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,offset,sk", [(37, 53, 1, "w+3"), (70, 512, 0, "w+4"), (31, 96, 2, "pitch"), (5, 3, 3, "2w"), (70, 520, 64, "w+1")])
def test_random_field_into_a_strided_buffer_leaves_the_gaps_alone(pkg, eng, h, w, offset, sk):
    import torch
    rs = strided.row_stride_of(sk, w)
    for sentinel in (0xA5, 0x00):
        host, off, mask = strided.embed(np.full((h, w), sentinel, np.uint8), offset, rs, 0xFF)
        host[mask] = sentinel
        t = torch.from_numpy(host).to(eng.device)
        assert pkg._ffi.lib().ws_random_field_device(eng.ctx.handle, t.data_ptr() + off, h, w, rs, 5) == 0
        _sync()
        back = t.cpu().numpy()
        assert (strided.view(back, off, h, w, rs) == ol.random_field(h, w, 5)).all()
        assert (back[mask] == sentinel).all()      # every gap and guard byte still holds the sentinel


# ---- 12. host ABI: the stride is consumed by a 2-D copy ---------------------------------------------------------------------------------------

def _host_view(img, offset, sk, fill):
    rs = strided.row_stride_of(sk, img.shape[1])
    backing, off, _ = strided.embed(img, offset, rs, fill)
    return backing, strided.view(backing, off, img.shape[0], img.shape[1], rs), rs


@pytest.mark.parametrize("offset,sk", [(1, "w+3"), (0, "pitch")])
def test_host_abi_on_strided_views(pkg, offset, sk):
    L = pkg._ffi.lib()
    ctx = pkg.api.Context(0)
    h, w = 70, 520
    img = cases.field(h, w, 81)
    seeds = np.asarray(ol.find_local_minima(img), dtype=np.uint64).reshape(-1, 2)
    levels = np.asarray([254, 3, 120], dtype=np.uint8)
    for edge in (False, True):
        opt = _opt(pkg, 254, edge)
        x = 2 if edge else 0
        res = []
        for fill in FILLS:
            backing, v, rs = _host_view(img, offset, sk, fill)
            keep = backing.copy()
            out = np.zeros((h + x, w + x), dtype=np.uint64)
            lst = np.zeros((len(seeds) + 8, 2), dtype=np.uint64)
            n = ctypes.c_size_t(0)
            assert L.ws_segment_minima(ctx.handle, v.ctypes.data, h, w, rs, ctypes.byref(opt), out.ctypes.data, lst.ctypes.data, len(lst), ctypes.byref(n)) == 0
            cap = len(seeds) * 255 + 16
            lakes = np.zeros((cap, 2), dtype=np.uint64)
            offsets, unc, nl = np.zeros(256, dtype=np.uint64), np.zeros(255, dtype=np.uint64), ctypes.c_size_t(0)
            assert L.ws_transform_to_list(ctx.handle, 1, v.ctypes.data, h, w, rs, seeds.ctypes.data, len(seeds), ctypes.byref(opt), lakes.ctypes.data, cap,
                                          ctypes.byref(nl), offsets.ctypes.data, unc.ctypes.data) == 0
            hist = np.zeros((3, h + x, w + x), dtype=np.uint64)
            assert L.ws_transform_history(ctx.handle, 0, v.ctypes.data, h, w, rs, seeds.ctypes.data, len(seeds), ctypes.byref(opt), levels.ctypes.data, 3,
                                          hist.ctypes.data) == 0
            assert (backing == keep).all()
            res.append((n.value, out, lst[: n.value].copy(), _records(lakes[: nl.value], offsets, unc, 0, 255), hist))
        assert _same(res[0], res[1])
        n, out, lst, recs, hist = res[0]
        assert n == len(seeds) and (lst == seeds).all() and (out == ol.segment_arrival(img, seeds, edge=edge)).all()
        _lists_equal(recs, _oracle_lists(img, seeds, True, 254, edge))
        assert (hist == _oracle_levels(img, seeds, False, list(levels), edge=edge)).all()
    ctx.close()


@pytest.mark.parametrize("offset,rs_extra,slice_gap", [(3, 5, 7), (0, 4, 0), (1, 0, 1)])
def test_host_abi_cubes_with_row_and_slice_gaps(pkg, offset, rs_extra, slice_gap):
    L = pkg._ffi.lib()
    ctx = pkg.api.Context(0)
    s, h, w = 4, 32, 96
    cube, lists, offs = _cube_case(s, h, w, 1500)
    flat = np.ascontiguousarray(np.concatenate(lists))
    rs, ss = w + rs_extra, h * (w + rs_extra) + slice_gap
    c_offs = _c_offsets(offs)
    for edge in (False, True):
        opt = _opt(pkg, 90, edge)
        x = 2 if edge else 0
        res = []
        for fill in FILLS:
            backing, off, _ = strided.embed_cube(cube, offset, rs, ss, fill)
            keep = backing.copy()
            base = backing.ctypes.data + off
            out = np.zeros((s, h + x, w + x), dtype=np.uint64)
            failed = ctypes.c_size_t(99)
            assert L.ws_segment_batch(ctx.handle, base, s, h, w, rs, ss, flat.ctypes.data, c_offs, ctypes.byref(opt), out.ctypes.data, None, ctypes.byref(failed)) == 0
            out2 = np.zeros((s, h + x, w + x), dtype=np.uint64)
            counts = (ctypes.c_size_t * s)()
            assert L.ws_segment_batch(ctx.handle, base, s, h, w, rs, ss, None, None, ctypes.byref(opt), out2.ctypes.data, counts, ctypes.byref(failed)) == 0
            cap = offs[-1] * 91 + 16
            lakes = np.zeros((cap, 2), dtype=np.uint64)
            offsets, unc, nl = np.zeros(s * 91 + 1, dtype=np.uint64), np.zeros(s * 91, dtype=np.uint64), ctypes.c_size_t(0)
            assert L.ws_transform_to_list_batch(ctx.handle, 0, base, s, h, w, rs, ss, flat.ctypes.data, c_offs, ctypes.byref(opt), lakes.ctypes.data, cap,
                                                ctypes.byref(nl), offsets.ctypes.data, unc.ctypes.data, None, ctypes.byref(failed)) == 0
            assert (backing == keep).all()
            res.append((out, out2, list(counts), [_records(lakes[: nl.value], offsets, unc, k, 91) for k in range(s)]))
        assert _same(res[0], res[1])
        out, out2, counts, recs = res[0]
        assert counts == [len(l) for l in lists]
        for k in range(s):
            want = ol.segment_arrival(cube[k], lists[k], max_level=90, edge=edge)
            assert (out[k] == want).all() and (out2[k] == want).all(), k
            _lists_equal(recs[k], _oracle_lists(cube[k], lists[k], False, 90, edge))
    ctx.close()


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("offset,sk", [(1, "w+3"), (0, "pitch")])
def test_host_abi_tiled_forms_on_strided_views(pkg, offset, sk, edge):
    # with edge correction the padded uploads of ws_segment_tiled / ws_segment_tiled2d index the source by hand
    L = pkg._ffi.lib()
    grp_mod = importlib.import_module("rustronomy_watershed_amd.group")
    h, w = 120, 300
    img = cases.smooth_field(h, w, 91)
    seeds = np.asarray(ol.find_local_minima(img), dtype=np.uint64).reshape(-1, 2)
    want = ol.segment_arrival(img, seeds, edge=edge)
    opt = _opt(pkg, 254, edge)
    x = 2 if edge else 0
    for fill in FILLS:
        backing, v, rs = _host_view(img, offset, sk, fill)
        keep = backing.copy()
        g = grp_mod.Group.local(2)
        out = np.zeros((h + x, w + x), dtype=np.uint64)
        rc = L.ws_segment_tiled(g._h, v.ctypes.data, h, w, rs, seeds.ctypes.data, len(seeds), ctypes.byref(opt), 0, out.ctypes.data, None)
        assert rc == 0, (rc, L.ws_group_last_error(g._h))
        assert (out == want).all(), ("row blocks", hex(fill))
        out = np.zeros((h + x, w + x), dtype=np.uint64)
        rc = L.ws_segment_tiled2d(g._h, v.ctypes.data, h, w, rs, seeds.ctypes.data, len(seeds), ctypes.byref(opt), 1, 2, 0, out.ctypes.data, None)
        assert rc == 0, (rc, L.ws_group_last_error(g._h))
        assert (out == want).all(), ("2-D tiles", hex(fill))
        g.close()
        assert (backing == keep).all()


# ---- 13. refusals before any launch ---------------------------------------------------------------------------------------------------------

def test_short_strides_are_refused_before_anything_runs(pkg):
    import torch
    e = _new_engine()
    L, ffi = pkg._ffi.lib(), pkg._ffi
    BAD = ffi.WS_ERR_BAD_ARG
    hnd = e.ctx.handle
    s, h, w = 3, 32, 96
    cube, lists, offs = _cube_case(s, h, w, 1600)
    c = Cube(e, cube, 0, w, h * w, 0xFF)
    seeds = _dev_seeds(e, lists[0])
    all_seeds = _dev_seeds(e, np.concatenate(lists))
    ns = len(lists[0])
    opt = _opt(pkg, 254)
    SENT = 0x5A5A5A5A
    lab = torch.full((s, 2, h, w), SENT, dtype=torch.int32, device=e.device)      # every output goes here
    n = ctypes.c_size_t(0)
    o, u = np.zeros(s * 255 + 1, dtype=np.uint64), np.zeros(s * 255, dtype=np.uint64)
    lv = np.asarray([0, 254], dtype=np.uint8)
    failed = ctypes.c_size_t(0)
    short = w - 1
    assert L.ws_find_local_minima_device(hnd, c.ptr, h, w, short, lab.data_ptr(), 16, ctypes.byref(n)) == BAD
    for fn in (L.ws_segment_device, L.ws_merge_device):
        assert fn(hnd, c.ptr, h, w, short, seeds.data_ptr(), ns, ctypes.byref(opt), lab.data_ptr()) == BAD, fn.__name__
    # (a transform that cannot be left in flight runs -- or is refused -- inside _begin, and _end hands its status over)
    for begin, end in ((L.ws_segment_device_begin, L.ws_segment_device_end), (L.ws_merge_device_begin, L.ws_merge_device_end)):
        assert (begin(hnd, c.ptr, h, w, short, seeds.data_ptr(), ns, ctypes.byref(opt), lab.data_ptr()) or end(hnd)) == BAD, begin.__name__
    assert L.ws_segment_minima_device(hnd, c.ptr, h, w, short, ctypes.byref(opt), lab.data_ptr(), None, 0, ctypes.byref(n)) == BAD
    for merging in (0, 1):
        assert L.ws_transform_to_list_device(hnd, merging, c.ptr, h, w, short, seeds.data_ptr(), ns, ctypes.byref(opt), lab.data_ptr(), 64, ctypes.byref(n),
                                             o.ctypes.data, u.ctypes.data) == BAD
        assert L.ws_transform_history_device(hnd, merging, c.ptr, h, w, short, seeds.data_ptr(), ns, ctypes.byref(opt), lv.ctypes.data, 2, lab.data_ptr(), h * w) == BAD
    assert L.ws_block_begin(hnd, c.ptr, h, w, short, 254, seeds.data_ptr(), ns, 1, lab.data_ptr()) == BAD
    assert L.ws_block_relax_halo(hnd, c.ptr, h, w, short, 254, 1, 1, lab.data_ptr()) == BAD
    # cubes: a short row stride, and slices that would overlap
    for rs, ss in ((short, h * w), (w, h * w - 1), (w + 4, h * (w + 4) - 1)):
        offsets = _c_offsets(offs)
        assert L.ws_segment_batch_device(hnd, c.ptr, s, h, w, rs, ss, all_seeds.data_ptr(), offsets, ctypes.byref(opt), lab.data_ptr(), ctypes.byref(failed)) == BAD
        assert L.ws_merge_batch_device(hnd, c.ptr, s, h, w, rs, ss, all_seeds.data_ptr(), offsets, ctypes.byref(opt), lab.data_ptr(), ctypes.byref(failed)) == BAD
        assert L.ws_transform_to_list_batch_device(hnd, 1, c.ptr, s, h, w, rs, ss, all_seeds.data_ptr(), offsets, ctypes.byref(opt), lab.data_ptr(), 64,
                                                   ctypes.byref(n), o.ctypes.data, u.ctypes.data, ctypes.byref(failed)) == BAD
        assert L.ws_transform_history_batch_device(hnd, 0, c.ptr, s, h, w, rs, ss, all_seeds.data_ptr(), offsets, ctypes.byref(opt), lv.ctypes.data, 2,
                                                   lab.data_ptr(), h * w, ctypes.byref(failed)) == BAD
    # a tile whose img_stride is shorter than the tile
    grp_mod = importlib.import_module("rustronomy_watershed_amd.group")
    g = grp_mod.Group.local(2)
    field = torch.zeros((64, 64), dtype=torch.uint8, device=e.device)
    blocks, _, _keep = g.make_blocks2d(field, torch.zeros((0, 2), dtype=torch.int32, device=e.device), 1, 2)
    blocks[1].img_stride = 8
    topt = ffi.Options(254)
    assert L.ws_segment_tiled2d_device(g._h, 64, 64, 1, 2, 0, blocks, ctypes.byref(topt), 0, None) == BAD
    g.close()
    _sync()
    assert bool((lab == SENT).all())      # refused before anything ran
    assert c.unchanged()
    # ... and the context is usable afterwards
    rc, got = _segment(pkg, e, c.ptr, h, w, w, lists[0], opt)
    assert rc == 0 and (got == ol.segment_arrival(cube[0], lists[0])).all()


# ---- 14. a row stride beyond 32 bits ----------------------------------------------------------------------------------------------------------

def test_row_stride_beyond_32_bits(pkg, eng):
    # k_relax's fast paths do their address arithmetic in 32 bits and are only taken for img_stride <= 2^32 - 1
    import torch
    free, _total = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        print(f"skipped: {free / 2 ** 30:.1f} GiB of device memory free, the 8 GiB backing array wants 12")
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, the 8 GiB backing array wants 12")
    h, w = 3, 512
    rs = 2 ** 32 + 4
    img = cases.field(h, w, 99)
    img[1, 100] = 254      # (a strict maximum in the one interior row, whatever the generator drew)
    seeds = np.asarray(ol.find_local_minima(img), dtype=np.uint64).reshape(-1, 2)
    assert len(seeds)
    want = ol.segment_arrival(img, seeds)
    hood = 4096
    t = torch.empty(strided.plane_bytes(h, w, 0, rs), dtype=torch.uint8, device=eng.device)
    assert t.data_ptr() % 256 == 0
    results = []
    for fill in FILLS:
        for y in range(h):      # only the three rows and a neighbourhood of each are written
            p = strided.GUARD + y * rs
            t[p - hood: p + w + hood] = fill
            t[p: p + w] = torch.from_numpy(img[y]).to(eng.device)
        ptr = t.data_ptr() + strided.GUARD
        rc, n, out = _minima(pkg, eng, ptr, h, w, rs)
        assert rc == 0 and n == len(seeds) and (out[:n] == seeds.astype(np.int64)).all()
        for engine in (pkg.ENGINE_FUSED, pkg.ENGINE_SWEEP):
            rc, got = _segment(pkg, eng, ptr, h, w, rs, seeds, _opt(pkg, 254, False, engine))
            assert rc == 0 and (got == want).all(), (hex(fill), engine)
            results.append(got)
        for y in range(h):
            p = strided.GUARD + y * rs
            assert bool((t[p: p + w].cpu() == torch.from_numpy(img[y])).all())
            assert bool((t[p - hood: p] == fill).all()) and bool((t[p + w: p + w + hood] == fill).all())
    del t
    torch.cuda.empty_cache()
