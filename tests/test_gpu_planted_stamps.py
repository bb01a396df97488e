"""The relaxation kernels from planted stamp planes, and the ring-overflow status (-m gpu).

Every other GPU test of ws_relax.hip starts from seeds: the stamps the kernels see are the ones a flood from key 0 leaves,
rings of a few thousand at the most.  Here the start plane is planted (tests/planted_cases.py) and the answer is the exact
fixpoint of a heap Dijkstra without a ring field (planted_cases.planted_fixpoint; tests/test_planted_cases_cpu.py proves the
families on the CPU):

  ws_block_relax          takes the caller's d_keys as the start state: pass 0 is a FULL launch without seeds that runs every
                          tile, the later passes walk FULL_LITE, CHUNKED, CHUNKED_SCAN, LISTED, LIST_REGRID / LISTED_SPLIT with
                          append (ws_relax_plan.hpp), with the carry test in every write-back
  ws_block_begin + ws_block_relax_halo
                          the same from the caller's halo rows, from pass 4 on (scan variants only); the carry test is left to
                          ws_block_resolve_local
  ws_block_resolve_ring   any finished plane

rows / columns put a blocker -- a higher level, a wall, a wall between two fronts -- at every lane position where scan_row hands
over (DPP row ends, row_bcast, v_readlane at lanes 16 / 32 / 48, the half rows of the SPLIT kernel) and at every patch row of
every band of scan_cols_both, in both directions; the high-ring forms run stamps that end exactly on the last ring the
contract allows through the same scans at levels 7, 253 (max_level 253: the other patch_bases path) and 254; the overflow
twins need one ring more at exactly one pixel and must be refused with WS_ERR_RING_OVERFLOW, at level 254 too, where the
carry itself is KEY_INF and shows nowhere.  A stamp that comes out too LOW is permanent (stamps only fall): every plane is
compared bit for bit.

Out of reach of planted stamps: k_relax0_tall, k_relax_strips_tall and the queue kernels need a seed plane or persist_mode,
which the block calls do not set.  The queue kernels (k_relax, PERSIST 1 and 2: 128 x 128 tiles, 32 bands) have corridors of
their own, flooded from seeds, in tests/test_gpu_queue_corridors.py (tests/queue_cases.py).

Relaxation passes observed (ws_ctx_get_stats; pass_loop launches passes in groups of 2, 1, 2, 4, 8, 16 and counts what it
launched, so the values are 3, 5, 9, 17, 33: 33 = the first pass that changed nothing was one of 9 .. 16, past pass 7, the
first LISTED_SPLIT):
  ws_block_relax       rows/776 33, rows/774 33, columns/260 33, high/rows/* 33, high/columns/* 33; random/* 5 or 9 (the first
                       clean pass was 2, 3 or 4: those planes exercise the early variants and the arithmetic, not the scans)
  ws_block_relax_halo  columns/260 17, high/columns/* 17 (passes 4 .. 20 launched)
With the half-row select of scan_row taken out for the sweep to the right (lane 32 of the SPLIT kernel then takes what leaves
lane 31, a row of another band) rows/776, rows/774 and high/rows/* fail -- 15 312 wrong pixels in rows/776 -- and every random
plane still passes: the corridors are what proves the scans.
"""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import planted_cases as pc

pytestmark = pytest.mark.gpu

CORRIDORS = tuple(n for n in pc.SOUND if not n.startswith("random/"))
FAST = tuple(n for n in pc.SOUND if "columns" in n)      # W % 4 == 0 and stamps on the first and last row only


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def eng(pkg):
    return importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


def _new_engine():
    return importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


def _dev(e, a):
    import torch
    a = np.array(a, copy=True)      # (the cases are read-only arrays)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(e.device)


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _passes(e):
    return e.ctx.stats()["relax_passes"]


def _relax(pkg, e, d_img, d_keys, max_level):
    h, w = d_keys.shape
    chg = ctypes.c_int(-1)
    rc = pkg._ffi.lib().ws_block_relax(e.ctx.handle, d_img.data_ptr(), h, w, w, max_level, d_keys.data_ptr(), ctypes.byref(chg))
    return rc, chg.value


def _relax_sound(pkg, e, name):
    """One sound case through ws_block_relax: the exact plane, changed == 1, and a second call that finds nothing."""
    img, t0, ml = pc.CASES[name]()
    want, overflow = pc.reference(name)
    assert not overflow
    d_img, d_keys = _dev(e, img), _dev(e, t0)
    before = _passes(e)
    rc, changed = _relax(pkg, e, d_img, d_keys, ml)
    passes = _passes(e) - before
    got = _host(d_keys)
    print(f"{name}: ws_block_relax rc {rc} changed {changed} passes {passes} wrong pixels {int((got != want).sum())}")
    assert rc == pkg._ffi.WS_OK and changed == 1
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, len(bad), [(int(y), int(x), hex(got[y, x]), hex(want[y, x])) for y, x in bad[:8]])
    rc, changed = _relax(pkg, e, d_img, d_keys, ml)
    assert rc == pkg._ffi.WS_OK and changed == 0
    assert (_host(d_keys) == want).all()
    return passes


def _fast_form(pkg, e, name):
    """ws_block_begin without seeds, the halo rows overwritten with the planted stamps, ws_block_relax_halo, then
    ws_block_resolve_local.  -> (statuses, plane after the repair, its passes)"""
    import torch
    L = pkg._ffi.lib()
    img, t0, ml = pc.CASES[name]()
    h, w = img.shape
    assert w % 4 == 0 and (t0[1:-1] == pc.KEY_INF).all()
    d_img = _dev(e, img)
    d_keys = torch.zeros((h, w), dtype=torch.int32, device=e.device)
    d_labels = torch.zeros((h, w), dtype=torch.int32, device=e.device)
    rc = [L.ws_block_begin(e.ctx.handle, d_img.data_ptr(), h, w, w, ml, None, 0, 1, d_keys.data_ptr())]
    assert (_host(d_keys) == pc.KEY_INF).all()      # no seeds: nothing was coloured
    d_keys[0] = _dev(e, t0[0])
    d_keys[h - 1] = _dev(e, t0[h - 1])
    assert (_host(d_keys) == t0).all()              # the plane the reference was taken from
    rc.append(L.ws_block_relax_halo(e.ctx.handle, d_img.data_ptr(), h, w, w, ml, 1, 1, d_keys.data_ptr()))
    passes = _passes(e)                             # (the fast calls restart the counters: the value is this call's own)
    got = _host(d_keys).copy()
    rc.append(L.ws_block_resolve_local(e.ctx.handle, d_keys.data_ptr(), d_labels.data_ptr(), h, w, 1, 1))
    print(f"{name}: begin / relax_halo / resolve_local rc {rc} passes {passes}")
    return rc, got, passes


@pytest.mark.parametrize("name", pc.SOUND)
def test_block_relax_reaches_the_fixpoint_of_a_planted_plane(pkg, eng, name):
    passes = _relax_sound(pkg, eng, name)
    if name in CORRIDORS:
        assert passes >= 8, (name, passes)      # pass 7 is the first LISTED_SPLIT (relax_plan with the product's knobs)


@pytest.mark.parametrize("name", FAST)
def test_relax_halo_reaches_the_fixpoint_from_planted_halo_rows(pkg, eng, name):
    want, overflow = pc.reference(name)
    assert not overflow
    rc, got, passes = _fast_form(pkg, eng, name)
    ok = pkg._ffi.WS_OK
    assert rc == [ok, ok, ok]
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, len(bad), [(int(y), int(x), hex(got[y, x]), hex(want[y, x])) for y, x in bad[:8]])
    assert passes >= 1


@pytest.mark.parametrize("name", pc.TWINS)
def test_block_relax_refuses_the_overflow_twin_and_the_flag_does_not_stick(pkg, name):
    e = _new_engine()
    img, t0, ml = pc.CASES[name]()
    assert pc.reference(name)[1]
    d_img, d_keys = _dev(e, img), _dev(e, t0)
    rc, _ = _relax(pkg, e, d_img, d_keys, ml)
    print(f"{name}: ws_block_relax rc {rc}")
    assert rc == pkg._ffi.WS_ERR_RING_OVERFLOW
    assert b"ring" in pkg._ffi.lib().ws_last_error(e.ctx.handle)
    _relax_sound(pkg, e, name.replace("twin/", "high/"))


@pytest.mark.parametrize("name", [n for n in pc.TWINS if "columns" in n])
def test_resolve_local_refuses_the_overflow_twin_after_relax_halo(pkg, name):
    e = _new_engine()
    ok = pkg._ffi.WS_OK
    rc, _, _ = _fast_form(pkg, e, name)
    assert rc == [ok, ok, pkg._ffi.WS_ERR_RING_OVERFLOW]
    sound = name.replace("twin/", "high/")
    rc, got, _ = _fast_form(pkg, e, sound)
    assert rc == [ok, ok, ok]
    assert (got == pc.reference(sound)[0]).all()


@pytest.mark.parametrize("name", pc.TWINS)
def test_resolve_ring_refuses_a_finished_plane_past_the_last_ring(pkg, name):
    import torch
    e = _new_engine()
    L = pkg._ffi.lib()
    plane, overflow = pc.reference(name)      # the reference's stamps in 32 bits
    assert overflow
    h, w = plane.shape
    d_labels = torch.zeros((h, w), dtype=torch.int32, device=e.device)
    d_keys = _dev(e, plane)
    rc = L.ws_block_resolve_ring(e.ctx.handle, d_keys.data_ptr(), d_labels.data_ptr(), h, w)
    print(f"{name}: ws_block_resolve_ring rc {rc}")
    assert rc == pkg._ffi.WS_ERR_RING_OVERFLOW
    sound, _ = pc.reference(name.replace("twin/", "high/"))
    d_keys = _dev(e, sound)
    assert L.ws_block_resolve_ring(e.ctx.handle, d_keys.data_ptr(), d_labels.data_ptr(), h, w) == pkg._ffi.WS_OK
    assert (_host(d_keys) == sound).all()
