"""The two-launch label resolve (csrc/ws_resolve.hip): every instantiation of k_resolve_local on every load / store
form, and the chase's dense path, bit for bit against the oracle.

resolve_two_launch picks the instantiation from the ResolveJob; the kernels pick their code by the plane:

  seed list sorted         -> TABLES (colours from the side tables)       ws_segment_device, sorted list
  seed list shuffled       -> painted labels                              ws_segment_device, shuffled list
  ws_merge_device          -> + MERGE (tile_min)                          both lists
  row blocks of a field    -> TABLES + BLOCK (halo rows; w % 4 == 0 only) ws_segment_tiled on a local group
  2 x 2 tiles of a field   -> BLOCK alone (the ring form, painted)        ws_segment_tiled2d_device (both access forms)
  W % 4 == 0, planes 16-byte aligned -> 16-byte accesses, else 4-byte ones; a tile wholly inside the plane skips the masks
  a wave with >= 256 references writes no list: the chase reads its 64 x 16 pixels from the plane (dense path) and, on
  a plane without halo rows, compresses chains of more than three hops

The CPU half (not marked gpu) derives each case's regime from the oracle's arrival stamps alone -- references per wave
region, chain length in tiles, one-lake and hole tiles -- so that a GPU test cannot pass on an input that misses it."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import oracle_lib as ol

TS, REGION_ROWS, REF_DENSE = 64, 16, 256
NEVER = np.uint64(0xFFFFFFFFFFFFFFFF)

# the smallest shapes that reach each form: one whole tile; W % 4 != 0 with partial tiles both ways and a second tile
# column 3 wide; 16-byte form with partial tiles
SHAPES = [(64, 64), (61, 67), (130, 132)]


# ---- CPU side: the forest the oracle's stamps define, cut into the kernel's tiles ------------------------------------------------

def _seeds_of(img):
    return np.ascontiguousarray(np.asarray(ol.find_local_minima(img), dtype=np.uint64).reshape(-1, 2))


def _shuffled(seeds, k):
    return np.ascontiguousarray(seeds[np.random.default_rng(k).permutation(len(seeds))])


def strictly_increasing(seeds, w):
    """the condition that selects the seed tables (TABLES) over painted labels: row-major pixel indices strictly increasing"""
    pos = seeds[:, 0].astype(np.int64) * w + seeds[:, 1].astype(np.int64)
    return bool((np.diff(pos) > 0).all())


# the row-block cases (h, w, virtual ranks): the fast block form, hence TABLES + BLOCK, needs a strictly increasing list,
# w % 4 == 0 and blocks of at least two rows (block_check, csrc/ws_block_api.hip); anything else falls back to the iterative form
ROW_BLOCKS = [(130, 132, 2), (192, 64, 3)]


def regime(img, seeds):
    """From ol.segment_arrival alone: per pixel, is its label a reference after k_resolve_local (its parent chain leaves
    its 64 x 64 tile), and over how many tiles its chain runs; per 64 x 16 wave region the number of references."""
    labels, keys = ol.segment_arrival(img, seeds, want_keys=True)
    h, w = keys.shape
    n = h * w
    idx = np.arange(n, dtype=np.int64).reshape(h, w)
    pad = np.full((h + 2, w + 2), NEVER, dtype=np.uint64)
    pad[1:-1, 1:-1] = keys
    k = keys
    d, r, l = pad[2:, 1:-1] < k, pad[1:-1, 2:] < k, pad[1:-1, :-2] < k
    flooded = (k != 0) & (k != NEVER)
    par = np.where(d, idx + w, np.where(r, idx + 1, np.where(l, idx - 1, idx - w)))      # first earlier neighbour in D, R, L, U
    par = np.where(flooded, par, idx).ravel()
    assert (keys.ravel()[par[flooded.ravel()]] < keys.ravel()[flooded.ravel()]).all()      # a fixpoint: a parent is earlier
    tile = ((idx // w) // TS * ((w + TS - 1) // TS) + (idx % w) // TS).ravel()
    flat = idx.ravel()
    nxt = np.where(tile[par] == tile, par, flat)      # the in-tile forest; pointer jumping as the kernel does it
    while True:
        nn = nxt[nxt]
        if (nn == nxt).all():
            break
        nxt = nn
    is_ref = par[nxt] != nxt                              # the in-tile root's parent lies in another tile
    leaves_to = par[nxt]
    hops = np.zeros(n, dtype=np.int64)                    # tiles a chain is followed through by the chase
    cur = flat.copy()
    while True:
        go = is_ref[cur]
        if not go.any():
            break
        hops += go
        cur = np.where(go, leaves_to[cur], cur)
    ref2d = is_ref.reshape(h, w)
    regions = {}
    for ty in range((h + TS - 1) // TS):
        for tx in range((w + TS - 1) // TS):
            for band in range(TS // REGION_ROWS):
                y0 = ty * TS + band * REGION_ROWS
                regions[(ty, tx, band)] = int(ref2d[y0:y0 + REGION_ROWS, tx * TS:(tx + 1) * TS].sum())
    return {"labels": labels, "is_ref": ref2d, "hops": hops.reshape(h, w), "regions": regions}


@functools.lru_cache(maxsize=None)
def shape_case(h, w):
    img = cases.field(h, w, 90 + h + w)
    return img, _seeds_of(img)


@functools.lru_cache(maxsize=None)
def ramp_case():
    """A monotone 192 x 256 ramp with one seed in a corner: every tile but the seed's is all references, and the chains
    run left along a row and then up the first column, through up to five tiles."""
    y, x = np.mgrid[0:192, 0:256]
    img = ((y + x) * 253 // (191 + 255)).astype(np.uint8)
    seeds = np.array([[1, 1]], dtype=np.uint64)
    reg = regime(img, seeds)
    for (ty, tx, band), cnt in reg["regions"].items():
        if (ty, tx) == (0, 0):
            assert cnt == 0                               # the seed's own tile resolves in LDS
        else:
            assert cnt >= REF_DENSE, (ty, tx, band, cnt)      # ... every other wave takes the REF_ALL path of the chase
    assert reg["hops"].max() > 3                          # follow_chain<true> compresses such a chain
    interior = np.zeros(img.shape, bool)
    interior[1:-1, 1:-1] = True
    for ty in range(3):                                   # merging: all coloured, all references -> RL_TILE_UNDECIDED
        for tx in range(4):
            if (ty, tx) != (0, 0):
                sl = (slice(ty * TS, (ty + 1) * TS), slice(tx * TS, (tx + 1) * TS))
                assert (reg["labels"][sl][interior[sl]] != 0).all() and reg["is_ref"][sl][interior[sl]].all()
    return img, seeds


@functools.lru_cache(maxsize=None)
def one_lake_case():
    """192 x 192 for the merging transform: the middle tile is one lake with a seed of its own, the tile left of it has a
    pixel that never floods (a hole: tile_min = 0)."""
    img = np.full((192, 192), 7, np.uint8)
    img[90:100, 90:100] = 3
    img[20:30, 150:160] = 3
    img[160:170, 20:30] = 5
    img[96, 32] = 255
    seeds = np.array([[25, 155], [95, 95], [165, 25]], dtype=np.uint64)
    reg = regime(img, seeds)
    mid = (slice(TS, 2 * TS), slice(TS, 2 * TS))
    assert (reg["labels"][mid] != 0).all() and (reg["labels"][mid] == 2).any()      # no hole, and a colour that needs no chase
    assert not reg["is_ref"][95, 95]
    left = reg["labels"][TS:2 * TS, 0:TS]
    assert left[32, 32] == 0 and (left[:, 1:] != 0).sum() == TS * (TS - 1) - 1      # exactly one interior hole
    return img, seeds


def test_the_oracle_puts_each_case_in_its_regime():
    ramp_case()
    one_lake_case()
    for h, w in SHAPES:
        img, seeds = shape_case(h, w)
        reg = regime(img, seeds)
        cnts = list(reg["regions"].values())
        assert len(seeds) > 4 and max(cnts) < REF_DENSE      # noise: work lists, never the dense path
        assert (max(cnts) > 0) == (h > TS or w > TS)          # (one tile that is the whole plane: no chain leaves it)
        assert strictly_increasing(seeds, w) and not strictly_increasing(_shuffled(seeds, h), w)      # tables / painted
        assert not strictly_increasing(_shuffled(seeds, 7), w) and not strictly_increasing(_shuffled(seeds, w), w)
    for img, seeds in (ramp_case(), one_lake_case()):
        assert strictly_increasing(seeds, img.shape[1])
    assert not strictly_increasing(one_lake_case()[1][[2, 0, 1]], 192)
    assert not strictly_increasing(np.concatenate([ramp_case()[1]] * 2), 256)      # the seed listed twice: painted
    for h, w, n_ranks in ROW_BLOCKS:
        assert (h, w) in SHAPES or w == TS      # (shape_case serves them)
        assert w % 4 == 0 and h // n_ranks >= 2 and strictly_increasing(shape_case(h, w)[1], w)
    # 61 x 67: the second tile column is 3 wide and the last row of tiles partial
    assert (67 + TS - 1) // TS == 2 and 67 - TS == 3 and 61 < TS


# ---- GPU side ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def eng(pkg):
    import torch
    with torch.cuda.stream(torch.cuda.Stream(0)):
        yield importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


def _dev(eng, img, seeds):
    import torch
    s = np.asarray(seeds, dtype=np.int64).reshape(-1, 2).astype(np.int32)
    return torch.from_numpy(np.ascontiguousarray(img)).to(eng.device), torch.from_numpy(s).to(eng.device).contiguous()


def _run(eng, img, seeds, merging):
    import torch
    d_img, d_seeds = _dev(eng, img, seeds)
    out = (eng.merge if merging else eng.segment)(d_img, d_seeds)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _want(img, seeds, merging):
    return ol.merge_arrival(img, seeds) if merging else ol.segment_arrival(img, seeds)


@pytest.mark.gpu
@pytest.mark.parametrize("merging", [False, True], ids=["segment", "merge"])
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("h,w", SHAPES)
def test_tables_and_painted_with_and_without_merge_on_every_load_store_form(eng, h, w, order, merging):
    img, seeds = shape_case(h, w)
    if order == "shuffled":
        seeds = _shuffled(seeds, h)
    got = _run(eng, img, seeds, merging)
    want = _want(img, seeds, merging)
    assert got.shape == want.shape and (got == want).all(), int((got != want).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["ws_segment_device", "ws_merge_device"])
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_label_plane_off_16_byte_alignment_takes_the_scalar_form(pkg, eng, order, fn):
    # W % 4 == 0, but the label plane starts 4 bytes past a 16-byte boundary: 4-byte loads and stores in both kernels
    import torch
    h, w = 130, 132
    img, seeds = shape_case(h, w)
    if order == "shuffled":
        seeds = _shuffled(seeds, 7)
    d_img, d_seeds = _dev(eng, img, seeds)
    buf = torch.full((h * w + 8,), 0x5A5A5A5A, dtype=torch.int32, device=eng.device)
    assert buf.data_ptr() % 16 == 0
    opt = pkg._ffi.Options(254, 0, 0, 0, 0)
    rc = getattr(pkg._ffi.lib(), fn)(eng.ctx.handle, d_img.data_ptr(), h, w, w, d_seeds.data_ptr(), len(seeds), ctypes.byref(opt),
                                     buf.data_ptr() + 4)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    want = _want(img, seeds, fn == "ws_merge_device")
    assert rc == 0 and (got[1:1 + h * w].reshape(h, w) == want).all()
    assert got[0] == 0x5A5A5A5A and (got[1 + h * w:] == 0x5A5A5A5A).all()      # nothing outside the plane was written


@pytest.mark.gpu
@pytest.mark.parametrize("merging,twice", [(False, False), (True, False), (False, True)], ids=["segment", "merge", "segment-painted"])
def test_dense_references_and_long_chains_on_a_ramp(eng, merging, twice):
    img, seeds = ramp_case()
    if twice:      # the seed listed twice: not strictly increasing, so the painted form; the later entry's colour wins
        seeds = np.ascontiguousarray(np.concatenate([seeds, seeds]))
    got = _run(eng, img, seeds, merging)
    assert (got == _want(img, seeds, merging)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_one_lake_tile_next_to_a_tile_with_a_hole(eng, order):
    img, seeds = one_lake_case()
    if order == "shuffled":
        seeds = np.ascontiguousarray(seeds[[2, 0, 1]])
    got = _run(eng, img, seeds, True)
    assert (got == ol.merge_arrival(img, seeds)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,n_ranks", ROW_BLOCKS)
def test_row_blocks_of_a_sorted_list_take_the_tables_block_form(pkg, h, w, n_ranks):
    # w % 4 == 0 and a strictly increasing list: ws_block_begin / _resolve_local on every virtual rank (halo rows top, bottom, both)
    img, seeds = shape_case(h, w)
    L = pkg._ffi.lib()
    g = ctypes.c_void_p()
    assert L.ws_group_create_local(n_ranks, None, ctypes.byref(g)) == 0
    try:
        out = np.zeros((h, w), dtype=np.uint64)
        opt = pkg._ffi.Options(254, 0, 0, 0, 0)
        rounds = ctypes.c_uint32(0)
        rc = L.ws_segment_tiled(g, np.ascontiguousarray(img).ctypes.data, h, w, w, seeds.ctypes.data, len(seeds), ctypes.byref(opt), 0,
                                out.ctypes.data, ctypes.byref(rounds))
        assert rc == 0, L.ws_group_last_error(g)
    finally:
        L.ws_group_destroy(g)
    assert (out == ol.segment_arrival(img, seeds)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(130, 132), (61, 67), (130, 134)])
def test_2_by_2_tiles_take_the_ring_form(pkg, h, w):
    # a tile's plane is its own columns and one halo column: 67 wide at w = 132 (4-byte form), 68 at w = 134 (16-byte form)
    import torch
    img, seeds = shape_case(h, w)
    seeds = _shuffled(seeds, w)
    grp = importlib.import_module("rustronomy_watershed_amd.group").Group.local(4)
    try:
        dev = torch.device("cuda", 0)
        field = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
        s = torch.from_numpy(seeds.astype(np.int64).astype(np.int32)).to(dev)
        blocks, spans, keep = grp.make_blocks2d(field, s, 2, 2)
        assert all((chi - clo) % 4 == 0 for _, (c0, c1, clo, chi), _ in spans) == (w == 134)
        assert any((chi - clo) % 4 == 0 for _, (c0, c1, clo, chi), _ in spans) == (w == 134)
        grp.segment_tiled2d_device(h, w, 2, 2, blocks, max_level=254, n_seeds_total=len(seeds), merging=False)
        torch.cuda.synchronize()
        got = np.zeros((h, w), dtype=np.uint32)
        for (r0, r1, lo, hi), (c0, c1, clo, chi), lab in spans:
            got[r0:r1, c0:c1] = lab.cpu().numpy().view(np.uint32)[r0 - lo:r1 - lo, c0 - clo:c1 - clo]
    finally:
        grp.close()
    assert (got == ol.segment_arrival(img, seeds)).all()
