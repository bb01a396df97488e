"""merge_tree and the lake catalogue of a field tiled over the ranks of a group (ws_merge_tree_tiled_device,
ws_merge_tree_tiled2d_device, ws_merge_tree_tiled), -m gpu: local groups of 1 to 8 ranks on device 0 and an RCCL group of one.
The flood runs on all ranks, the arrival planes are gathered on rank 0 and ws_merge_tree_from_arrival_device runs there; the
records must equal the single-context call's on the whole field bit for bit, and the records derived from the CPU oracle's
per-level planes (tests/merge_tree_ref.py, tests/lake_stats_ref.py).  Integers only, no tolerance."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import lake_stats_ref as ls
import merge_tree_ref as mt
import oracle_lib as ol
import tiled_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def eng(pkg):
    import torch
    with torch.cuda.stream(torch.cuda.Stream(0)):
        yield importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


@pytest.fixture(scope="module")
def groups(pkg):
    """One local group per world for the whole module, and ("rccl", 1): an RCCL group of one rank."""
    grp_mod = importlib.import_module("rustronomy_watershed_amd.group")
    gs = {world: grp_mod.Group.local(world) for world in (1, 2, 3, 4, 8)}
    gs["rccl"] = grp_mod.Group.rccl(0, 0, 1, lambda raw: raw)
    yield gs
    for g in gs.values():
        g.close()


def _np(t):
    return t.cpu().numpy()


def _u16(shape, seed):
    """A u16 weight plane that is no function of the image and holds 0 and 65535 several times each (ties at the peak)."""
    rng = np.random.default_rng(2000 + seed)
    wt = rng.integers(0, 65536, shape, dtype=np.uint16)
    flat = wt.reshape(-1)
    where = rng.permutation(flat.size)
    flat[where[:max(flat.size // 50, 2)]] = 65535
    flat[where[-max(flat.size // 50, 2):]] = 0
    return wt


def _w_dev(wt):
    import torch
    wt = np.ascontiguousarray(wt)
    return torch.from_numpy(wt if wt.dtype == np.uint8 else wt.view(np.int16)).to("cuda:0")


def _row_blocks(ffi, g, t_img, hseeds):
    """Descriptors of a field's row blocks for any seed list: a strictly increasing list as contiguous ranges (no colours: the
    fast form where the width allows it), any other list seed by seed with explicit colours (the general form)."""
    import torch
    H, W = t_img.shape
    fast = tc.is_strictly_increasing(hseeds, W)
    blocks = (ffi.TileBlock * g.n_local)()
    spans, keep = [], []
    for r in range(g.n_local):
        r0, r1, lo, hi = g.tile_rows(H, r, g.world)
        inside = (hseeds[:, 0] >= lo) & (hseeds[:, 0] < hi)
        idx = np.nonzero(inside)[0]
        loc = hseeds[inside].copy()
        loc[:, 0] -= lo
        t_loc = torch.from_numpy(loc.astype(np.int32)).to(t_img.device).contiguous()
        t_col = torch.from_numpy((idx + 1).astype(np.int32)).to(t_img.device).contiguous()
        bi = t_img[lo:hi].contiguous()
        lab = torch.full((hi - lo, W), -1, dtype=torch.int32, device=t_img.device)
        keep += [t_loc, t_col, bi, lab]
        spans.append((r0, r1, lo, lab))
        if fast:
            assert len(idx) == 0 or (np.diff(idx) == 1).all()
        blocks[r] = ffi.TileBlock(bi.data_ptr(), t_loc.data_ptr() if len(idx) else None, None if fast else (t_col.data_ptr() if len(idx) else None),
                                  len(idx), int(idx[0]) + 1 if fast and len(idx) else 1, 0, lab.data_ptr())
    torch.cuda.synchronize()
    return blocks, spans, keep


_ORACLE = {}


def _oracle(key, img, seeds, wt, max_level=254, edge=False, seed_shift=False):
    """(tree, records) by the oracle route, once per input."""
    if key not in _ORACLE:
        _ORACLE[key] = ls.expected(img, seeds, weights=wt, max_level=max_level, edge=edge, seed_shift=seed_shift)
    return _ORACLE[key]


def _check_row_blocks(pkg, eng, g, key, himg, hseeds, seed=0):
    import torch
    himg = np.ascontiguousarray(himg)
    hseeds = np.asarray(hseeds, dtype=np.int64).reshape(-1, 2)
    H, W = himg.shape
    wt = _u16((H, W), seed)
    t_img = torch.from_numpy(himg).to(eng.device)
    t_seeds = torch.from_numpy(hseeds.astype(np.int32)).to(eng.device)
    t_wt = _w_dev(wt)
    want_tree, want = eng.merge_tree_stats(t_img, t_seeds, weights=t_wt)
    blocks, spans, keep = _row_blocks(pkg._ffi, g, t_img, hseeds)
    tree, stats, _ = g.merge_tree_tiled_device(H, W, len(hseeds), blocks, weights=t_wt, want_stats=True)
    alone, none, _ = g.merge_tree_tiled_device(H, W, len(hseeds), blocks, device=eng.device)      # the tree alone
    torch.cuda.synchronize()
    assert none is None
    assert (_np(tree) == _np(want_tree)).all() and (_np(alone) == _np(want_tree)).all(), key
    assert (_np(stats) == _np(want)).all(), (key, ls.mismatch(ls.from_raw(_np(stats)), ls.from_raw(_np(want))))
    o_tree, o_rec = _oracle(key, himg, hseeds, wt)
    assert (_np(tree).view(np.uint32) == o_tree).all(), (key, "oracle tree")
    assert ls.mismatch(ls.from_raw(_np(stats)), o_rec) is None, (key, "oracle", ls.mismatch(ls.from_raw(_np(stats)), o_rec))
    seg = ol.segment_arrival(himg, hseeds.astype(np.uint64))      # the blocks hold the segmenting labels, halo rows included
    for r0, r1, lo, lab in spans:
        assert (_np(lab[r0 - lo:r1 - lo]).view(np.uint32) == seg[r0:r1]).all(), key


PLAIN = [c for c in tc.all_cases() if not tc.edge_options(c[0])[0]]


def test_the_cases_hold_fast_forms_and_general_twins():
    forms = [tc.form_of(c[0]) for c in PLAIN]
    assert forms.count("fast") >= 30 and {"shuffled", "wide", "dup"} <= set(forms)
    assert {c[3] for c in PLAIN} == {2, 3, 4, 8}


@pytest.mark.parametrize("case", PLAIN, ids=[c[0] for c in PLAIN])
def test_row_blocks_on_the_tiled_cases(pkg, eng, groups, case):
    name, img, seeds, world = case
    _check_row_blocks(pkg, eng, groups[world], name, img, seeds, seed=len(name))


@pytest.mark.parametrize("world", [1, 2, 3, 4, "rccl"])
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_row_blocks_on_fields(pkg, eng, groups, kind, world):
    himg = cases.field(300, 256, 31) if kind == "noise" else cases.smooth_field(280, 192, 12, octaves=4)
    _check_row_blocks(pkg, eng, groups[world], kind, himg, ol.find_local_minima(himg), seed=7)


@pytest.mark.parametrize("shape,py,px", [((150, 131), 2, 2), ((150, 131), 1, 3), ((150, 131), 3, 1), ((2, 2), 2, 2), ((3, 5), 2, 2)])
def test_2d_tiles(pkg, eng, groups, shape, py, px):
    import torch
    H, W = shape
    if H * W > 100:
        himg = cases.field(H, W, 77)
        hseeds = np.asarray(ol.find_local_minima(himg), dtype=np.int64).reshape(-1, 2)
        hseeds = hseeds[np.random.default_rng(4).permutation(len(hseeds))]
    else:
        rng = np.random.default_rng(H * 100 + W)
        himg = rng.integers(0, 200, shape, dtype=np.uint8)
        hseeds = np.unique(np.stack([rng.integers(0, H, 3), rng.integers(0, W, 3)], axis=1), axis=0).astype(np.int64)
    g = groups[py * px]
    wt = _u16(shape, 9)
    t_img = torch.from_numpy(himg).to(eng.device)
    t_seeds = torch.from_numpy(hseeds.astype(np.int32)).to(eng.device)
    t_wt = _w_dev(wt)
    want_tree, want = eng.merge_tree_stats(t_img, t_seeds, weights=t_wt)
    blocks, spans, keep = g.make_blocks2d(t_img, t_seeds, py, px)
    tree, stats, _ = g.merge_tree_tiled2d_device(H, W, py, px, len(hseeds), blocks, weights=t_wt, want_stats=True)
    torch.cuda.synchronize()
    assert (_np(tree) == _np(want_tree)).all(), (shape, py, px)
    assert (_np(stats) == _np(want)).all(), (shape, py, px, ls.mismatch(ls.from_raw(_np(stats)), ls.from_raw(_np(want))))
    o_tree, o_rec = _oracle(("2d", shape), himg, hseeds, wt)
    assert (_np(tree).view(np.uint32) == o_tree).all() and ls.mismatch(ls.from_raw(_np(stats)), o_rec) is None
    seg = ol.segment_arrival(himg, hseeds.astype(np.uint64))
    for (r0, r1, lo, hi), (c0, c1, clo, chi), lab in spans:
        assert (_np(lab[r0 - lo:r1 - lo, c0 - clo:c1 - clo]).view(np.uint32) == seg[r0:r1, c0:c1]).all()


# ---- host buffers -------------------------------------------------------------------------------------------------------------------

HOST_FIELD = cases.field(97, 120, 19)
_SINGLE = {}


def _host_single(pkg, img, seeds, wt, edge, shift):
    """ws_merge_tree_stats on one context: (tree (n + 1, 4) uint32, records)."""
    L, ffi = pkg._ffi.lib(), pkg._ffi
    if "ws" not in _SINGLE:
        _SINGLE["ws"] = pkg.api.TransformBuilder().build_merging()      # one context for the module
    ctx = _SINGLE["ws"]._ctx()
    n = len(seeds)
    tree = np.zeros((n + 1, 4), dtype=np.uint32)
    rec = np.zeros(n + 1, dtype=ls.DTYPE)
    opt = ffi.Options(254, int(edge), 0, 0, int(shift))
    dtype = 0 if wt is None else ffi.WS_DTYPES["uint8" if wt.dtype == np.uint8 else "uint16"]
    rc = L.ws_merge_tree_stats(ctx.handle, img.ctypes.data, img.shape[0], img.shape[1], img.shape[1], seeds.ctypes.data if n else None, n, ctypes.byref(opt),
                               wt.ctypes.data if wt is not None else None, dtype, img.shape[1], tree.ctypes.data, rec.ctypes.data, None)
    assert rc == 0, (rc, L.ws_last_error(ctx.handle))
    return tree, rec


@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("edge,shift", [(False, False), (True, False), (True, True)])
def test_host_form_equals_the_single_context_host_call(pkg, groups, world, edge, shift):
    L, ffi = pkg._ffi.lib(), pkg._ffi
    img = HOST_FIELD
    h, w = img.shape
    full = np.ascontiguousarray(np.asarray(ol.find_local_minima(img), dtype=np.uint64).reshape(-1, 2))
    third = np.ascontiguousarray(full[np.random.default_rng(6).permutation(len(full))][: len(full) // 3])
    g = groups[world]
    for tag, seeds in (("full", full), ("shuffled third", third)):
        n = len(seeds)
        for wt in (None, np.random.default_rng(8).integers(0, 256, (h, w), dtype=np.uint8), _u16((h, w), 8)):
            want_tree, want = _host_single(pkg, img, seeds, wt, edge, shift)
            tree = np.full((n + 1, 4), 7, dtype=np.uint32)
            rec = np.zeros(n + 1, dtype=ls.DTYPE)
            opt = ffi.Options(254, int(edge), 0, 0, int(shift))
            dtype = 0 if wt is None else ffi.WS_DTYPES["uint8" if wt.dtype == np.uint8 else "uint16"]
            rc = L.ws_merge_tree_tiled(g._h, img.ctypes.data, h, w, w, seeds.ctypes.data, n, ctypes.byref(opt), wt.ctypes.data if wt is not None else None,
                                       dtype, w, tree.ctypes.data, rec.ctypes.data, None)
            assert rc == 0, (rc, L.ws_group_last_error(g._h))
            assert (tree == want_tree).all(), (tag, world, edge, shift)
            assert ls.mismatch(rec, want) is None, (tag, world, edge, shift, ls.mismatch(rec, want))
        # the tree alone
        tree = np.full((n + 1, 4), 7, dtype=np.uint32)
        opt = ffi.Options(254, int(edge), 0, 0, int(shift))
        assert L.ws_merge_tree_tiled(g._h, img.ctypes.data, h, w, w, seeds.ctypes.data, n, ctypes.byref(opt), None, 0, 0, tree.ctypes.data, None, None) == 0
        assert (tree == want_tree).all()
    # ... and against the oracle route, once: a shifted list, the image weighing
    if edge and shift and world == 2:
        o_tree, o_rec = ls.expected(img, third.astype(np.int64), weights=None, edge=True, seed_shift=True)
        got_tree, got = _host_single(pkg, img, third, None, True, True)
        assert (got_tree == o_tree).all() and ls.mismatch(got, o_rec) is None


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals_and_a_good_call_on_the_same_group(pkg, eng, groups):
    import torch
    L, ffi = pkg._ffi.lib(), pkg._ffi
    himg = cases.field(40, 64, 3)
    hseeds = np.asarray(ol.find_local_minima(himg), dtype=np.int64).reshape(-1, 2)
    n = len(hseeds)
    H, W = himg.shape
    t_img = torch.from_numpy(himg).to(eng.device)
    t_seeds = torch.from_numpy(hseeds.astype(np.int32)).to(eng.device)
    t_wt = _w_dev(_u16((H, W), 1))
    u16 = ffi.WS_DTYPES["uint16"]
    tree = torch.full((n + 1, 4), 77, dtype=torch.int32, device=eng.device)
    stats = torch.full((n + 1, 9), 77, dtype=torch.int64, device=eng.device)
    g = groups[3]
    blocks, spans, keep = _row_blocks(ffi, g, t_img, hseeds)
    plain, edge = ffi.Options(254), ffi.Options(254, 1)

    def rows(opt, weight, dtype, d_stats, field_h=H):
        return L.ws_merge_tree_tiled_device(g._h, field_h, W, n, blocks, ctypes.byref(opt), weight, dtype, W, tree.data_ptr(), d_stats, None)

    assert rows(edge, t_wt.data_ptr(), u16, stats.data_ptr()) == ffi.WS_ERR_UNSUPPORTED          # edge correction: pad the field first
    assert rows(plain, None, u16, stats.data_ptr()) == ffi.WS_ERR_BAD_ARG                        # the catalogue without weights
    assert b"d_weight" in L.ws_group_last_error(g._h)
    assert rows(plain, t_wt.data_ptr(), ffi.WS_DTYPES["float32"], stats.data_ptr()) == ffi.WS_ERR_UNSUPPORTED
    assert rows(plain, t_wt.data_ptr(), u16, stats.data_ptr(), field_h=2) == ffi.WS_ERR_BAD_ARG  # fewer rows than ranks
    g4 = groups[4]
    b2, spans2, keep2 = g4.make_blocks2d(t_img, t_seeds, 2, 2)

    def tiles(g_, py, px, opt, weight, d_stats):
        return L.ws_merge_tree_tiled2d_device(g_._h, H, W, py, px, n, b2, ctypes.byref(opt), weight, u16, W, tree.data_ptr(), d_stats, None)

    assert tiles(g4, 2, 3, plain, t_wt.data_ptr(), stats.data_ptr()) == ffi.WS_ERR_BAD_ARG       # py * px != world
    assert tiles(g4, 2, 2, edge, t_wt.data_ptr(), stats.data_ptr()) == ffi.WS_ERR_UNSUPPORTED
    assert tiles(g4, 2, 2, plain, None, stats.data_ptr()) == ffi.WS_ERR_BAD_ARG
    # host form: the weights' type, and a field with fewer rows than ranks
    hs = np.ascontiguousarray(hseeds.astype(np.uint64))
    ht, hr = np.zeros((n + 1, 4), dtype=np.uint32), np.zeros(n + 1, dtype=ls.DTYPE)
    wt8 = np.zeros((H, W), dtype=np.uint8)
    assert L.ws_merge_tree_tiled(g._h, himg.ctypes.data, H, W, W, hs.ctypes.data, n, ctypes.byref(plain), wt8.ctypes.data, ffi.WS_DTYPES["float32"], W,
                                 ht.ctypes.data, hr.ctypes.data, None) == ffi.WS_ERR_UNSUPPORTED
    assert L.ws_merge_tree_tiled(g._h, himg.ctypes.data, 2, W, W, None, 0, ctypes.byref(plain), None, 0, 0, ht.ctypes.data, None, None) == ffi.WS_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert (_np(tree) == 77).all() and (_np(stats) == 77).all()
    # the same groups run good calls afterwards
    want_tree, want = eng.merge_tree_stats(t_img, t_seeds, weights=t_wt)
    assert rows(plain, t_wt.data_ptr(), u16, stats.data_ptr()) == 0, L.ws_group_last_error(g._h)
    torch.cuda.synchronize()
    assert (_np(tree) == _np(want_tree)).all() and (_np(stats) == _np(want)).all()
    tree.fill_(77)
    stats.fill_(77)
    assert tiles(g4, 2, 2, plain, t_wt.data_ptr(), stats.data_ptr()) == 0, L.ws_group_last_error(g4._h)
    torch.cuda.synchronize()
    assert (_np(tree) == _np(want_tree)).all() and (_np(stats) == _np(want)).all()
