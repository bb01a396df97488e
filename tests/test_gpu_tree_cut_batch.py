"""The cut catalogue of a cube of slices in one call (ws_tree_cut_catalogue_batch_device, ws_merge_tree_cut_catalogue_batch(_device)),
on the GPU.  Every comparison is bit for bit.  Expected values come from the oracle route (tests/tree_cut_batch_cases.py:
tests/tree_cut_catalogue_ref.py per slice, concatenated); the single GPU call on each slice alone is the second witness."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import lake_stats_ref as ls
import tree_cut_batch_cases as bc

pytestmark = pytest.mark.gpu

S32 = 0x5A5A5A5A


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module", autouse=True)
def stream(torch):
    with torch.cuda.stream(torch.cuda.Stream(0)):      # a stream of its own: the level loops are captured and replayed
        yield


@pytest.fixture(scope="module")
def eng(pkg):
    return importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


def _dev(torch, eng, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(eng.device)


def _err(pkg, eng):
    return pkg._ffi.lib().ws_last_error(eng.ctx.handle).decode()


def _pcuts(pkg, cuts):
    return [pkg.Cut(*c.key()) for c in cuts]


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _same(tag, got, want):
    bad = ls.mismatch(np.asarray(got), np.asarray(want))
    assert bad is None, (tag,) + bad


def _check(tag, cube, cuts, planes, lakes, region, offsets, hidden, hidden_stats):
    """The outputs of one cube call (device tensors / numpy; planes, region and hidden_stats may be None) against the reference:
    every slice's planes, then the concatenated lists, offsets, hidden counts, region records and hidden records."""
    per = cube.expected(cuts)
    w_lakes, w_region, w_offsets, w_hidden, w_hid = cube.expected_flat(cuts)
    if planes is not None:
        got = _u32(planes)
        assert got.shape == (cube.n_slices, len(cuts)) + tuple(cube.plane_shape)
        for k in range(cube.n_slices):
            for j in range(len(cuts)):
                assert (got[k, j] == per[k][0][j]).all(), (tag, "plane", k, cuts[j])
    assert (np.asarray(offsets) == w_offsets).all(), (tag, "offsets", offsets, w_offsets)
    assert (np.asarray(hidden) == w_hidden).all(), (tag, "hidden")
    got_lakes = lakes.cpu().numpy().view(np.uint64)
    assert got_lakes.shape == w_lakes.shape and (got_lakes == w_lakes).all(), (tag, "lakes")
    if region is not None:
        rec = ls.from_raw(region.cpu().numpy())
        _same((tag, "regions"), rec, w_region)
        assert (rec["reserved"] == 0).all()
    if hidden_stats is not None:
        _same((tag, "hidden records"), ls.from_raw(hidden_stats), w_hid)


def _oracle_inputs(torch, eng, cube):
    """(tree, stats, keys, labels, weights) of a cube on the device, all from the oracle: (A) needs no flood of the engine's."""
    return (_dev(torch, eng, cube.tree()), _dev(torch, eng, cube.stats_raw()), _dev(torch, eng, cube.keys()), _dev(torch, eng, cube.seg()),
            _dev(torch, eng, cube.plane_weights()))


def _engine_inputs(torch, eng, cube):
    flat = np.concatenate(cube.lists, axis=0) if sum(len(l) for l in cube.lists) else np.zeros((0, 2), np.int64)
    dcube = torch.from_numpy(np.stack(cube.imgs)).to(eng.device).contiguous()
    wt = _dev(torch, eng, cube.weights) if cube.weights is not None else None
    return dcube, torch.from_numpy(flat.astype(np.int32)).to(eng.device).contiguous(), cube.seed_offsets(), wt


# ---- (A): from records and planes in HBM -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", bc.STACKING + bc.LOOPING + bc.DEVICE_ONLY)
def test_device_form_against_reference_and_single_calls(pkg, torch, eng, name):
    cube = bc.cube(name)
    cuts = cube.cuts
    tree, stats, keys, labels, wt = _oracle_inputs(torch, eng, cube)
    got = eng.tree_cut_catalogue_batch(tree, keys, labels, cube.seed_offsets(), _pcuts(pkg, cuts), weights=wt, stats=stats)
    torch.cuda.synchronize()
    _check(name, cube, cuts, *got)
    planes, lakes, region, offsets, hidden, hidden_stats = got
    # the second witness: ws_tree_cut_catalogue_device on every slice alone
    first, k_cuts = cube.first_records(), len(cuts)
    for k, f in enumerate(cube.slices):
        one = eng.tree_cut_catalogue(tree[first[k]:first[k + 1]], keys[k], labels[k], _pcuts(pkg, cuts), wt[k], stats=stats[first[k]:first[k + 1]])
        torch.cuda.synchronize()
        lo, hi = int(offsets[k * k_cuts]), int(offsets[(k + 1) * k_cuts])
        assert torch.equal(planes[k], one[0]) and torch.equal(lakes[lo:hi], one[1]) and torch.equal(region[lo:hi], one[2]), (name, k)
        assert (offsets[k * k_cuts:(k + 1) * k_cuts + 1] - offsets[k * k_cuts] == one[3]).all(), (name, k)
        assert (hidden[k * k_cuts:(k + 1) * k_cuts] == one[4]).all() and (hidden_stats[k * k_cuts:(k + 1) * k_cuts] == one[5]).all(), (name, k)


def test_device_form_nullable_outputs(pkg, torch, eng):
    """No planes; no lists; nothing measured (the plain tree_cut of a cube: no weights, and without catalogue cuts no stats)."""
    cube = bc.cube("5x40x96")
    cuts = cube.cuts
    tree, stats, keys, labels, wt = _oracle_inputs(torch, eng, cube)
    offs = cube.seed_offsets()
    a = eng.tree_cut_catalogue_batch(tree, keys, labels, offs, _pcuts(pkg, cuts), weights=wt, stats=stats, want_planes=False)
    torch.cuda.synchronize()
    assert a[0] is None
    _check("no planes", cube, cuts, *a)
    b = eng.tree_cut_catalogue_batch(tree, keys, labels, offs, _pcuts(pkg, cuts), weights=wt, stats=stats, want_lakes=False)
    torch.cuda.synchronize()
    per = cube.expected(cuts)
    for k in range(cube.n_slices):
        for j in range(len(cuts)):
            assert (_u32(b[0])[k, j] == per[k][0][j]).all()
    _same("hidden alone", ls.from_raw(b[5]), cube.expected_flat(cuts)[4])
    plain = [c for c in cuts if not c.catalogue]
    c = eng.tree_cut_catalogue_batch(tree, keys, labels, offs, _pcuts(pkg, plain), measure=False)
    torch.cuda.synchronize()
    assert c[2] is None and c[5] is None
    _check("plain", cube, plain, *c)


def test_device_form_views_off_alignment_and_odd_strides(pkg, torch, eng):
    """Records, planes and outputs 4 bytes off 16-byte alignment, plane_stride and the weight strides odd."""
    cube = bc.cube("9x8x16")
    cuts = cube.cuts
    s, (h, w), k = cube.n_slices, cube.plane_shape, len(cuts)
    n = h * w
    tree, stats, keys, labels, wt = _oracle_inputs(torch, eng, cube)

    def off(t, words=1):
        buf = torch.empty(t.numel() + words, dtype=t.dtype, device=t.device)
        buf[words:] = t.reshape(-1)
        return buf[words:].view(t.shape)

    tree_o, keys_o, labels_o = off(tree.view(-1)).view(-1, 4), off(keys), off(labels)
    wbig = torch.zeros((s, h + 3, w + 5), dtype=wt.dtype, device=wt.device)
    wbig[:, :h, :w] = wt
    stride = n + 3
    out = torch.full((s * k * stride + 1,), S32, dtype=torch.int32, device=eng.device)
    cap = len(cube.expected_flat(cuts)[0])
    lakes = torch.empty((cap, 2), dtype=torch.int64, device=eng.device)
    region = torch.empty((cap, 9), dtype=torch.int64, device=eng.device)
    offsets, hidden = np.zeros(s * k + 1, np.uint64), np.zeros(s * k, np.uint64)
    hs = np.zeros((s * k, 9), np.int64)
    got = ctypes.c_size_t(0)
    offs = (ctypes.c_size_t * (s + 1))(*cube.seed_offsets())
    arr = _lake_cuts(pkg, cuts)
    rc = pkg._ffi.lib().ws_tree_cut_catalogue_batch_device(
        eng.ctx.handle, tree_o.data_ptr(), stats.data_ptr(), s, offs, keys_o.data_ptr(), labels_o.data_ptr(), h, w, wbig.data_ptr(),
        pkg._ffi.WS_DTYPES["uint8"], w + 5, (h + 3) * (w + 5), arr, k, out.data_ptr() + 4, stride, lakes.data_ptr(), region.data_ptr(), cap,
        ctypes.byref(got), offsets.ctypes.data, hidden.ctypes.data, hs.ctypes.data)
    torch.cuda.synchronize()
    assert rc == 0, _err(pkg, eng)
    planes = out[1:].view(s, k, stride)
    assert (planes[:, :, n:] == S32).all() and int(out[0]) == S32
    _check("views", cube, cuts, planes[:, :, :n].reshape(s, k, h, w).contiguous(), lakes[:got.value], region[:got.value], offsets, hidden, hs)


def _lake_cuts(pkg, cuts):
    arr = (pkg._ffi.LakeCut * max(len(cuts), 1))()
    for k, c in enumerate(cuts):
        arr[k].min_area, arr[k].min_leaves, arr[k].show_level, arr[k].merge_level, arr[k].min_sum_w, arr[k].min_w_max, arr[k].min_depth = c.key()
    return arr


def _tiled_expected(base, which, cuts):
    per = base.expected(cuts)
    k = len(cuts)
    counts = np.array([[int(p[3][j + 1] - p[3][j]) for j in range(k)] for p in per])      # records of (distinct slice, cut)
    offsets = np.concatenate([[0], np.cumsum(counts[which].reshape(-1))]).astype(np.uint64)
    hidden = np.stack([p[4] for p in per])[which].reshape(-1).astype(np.uint64)
    return per, offsets, hidden


def test_65537_slices_meet_no_grid_limit(pkg, torch, eng):
    """65 537 slices of 8 x 16 tiled from three distinct ones, two cuts, through (A) and (B): expected values from three oracle runs."""
    base, which, cuts = bc.tiled()
    s, k = len(which), len(cuts)
    per, w_offsets, w_hidden = _tiled_expected(base, which, cuts)
    idx = torch.from_numpy(which).to(eng.device)
    first = base.first_records()
    n_seeds = np.array([f.n_seeds for f in base.slices])[which]
    offs = np.concatenate([[0], np.cumsum(n_seeds)])
    tree_parts = [base.tree()[first[d]:first[d + 1]] for d in range(3)]
    stats_parts = [base.stats_raw()[first[d]:first[d + 1]] for d in range(3)]
    tree = _dev(torch, eng, np.concatenate([tree_parts[d] for d in which]))
    stats = _dev(torch, eng, np.concatenate([stats_parts[d] for d in which]))
    keys, labels, wt = _dev(torch, eng, base.keys())[idx].contiguous(), _dev(torch, eng, base.seg())[idx].contiguous(), _dev(torch, eng, base.plane_weights())[idx].contiguous()

    def check(tag, planes, lakes, region, offsets, hidden, hidden_stats):
        assert (np.asarray(offsets) == w_offsets).all() and (np.asarray(hidden) == w_hidden).all(), tag
        want_planes = _dev(torch, eng, np.stack([np.stack(p[0]) for p in per]))[idx]
        assert torch.equal(planes, want_planes), tag
        want_lakes = _dev(torch, eng, np.concatenate([per[d][1] for d in which]))
        assert torch.equal(lakes, want_lakes), tag
        want_region = np.concatenate([per[d][2] for d in which])
        _same((tag, "regions"), ls.from_raw(region.cpu().numpy()), want_region)
        _same((tag, "hidden records"), ls.from_raw(hidden_stats), np.stack([per[d][5] for d in range(3)])[which].reshape(-1))

    got = eng.tree_cut_catalogue_batch(tree, keys, labels, offs, _pcuts(pkg, cuts), weights=wt, stats=stats)
    torch.cuda.synchronize()
    check("A", *got)
    del got
    imgs = torch.from_numpy(np.stack(base.imgs)).to(eng.device)[idx].contiguous()
    seeds = torch.from_numpy(np.concatenate([base.lists[d] for d in which]).astype(np.int32)).to(eng.device)
    res = eng.merge_tree_cut_catalogue_batch(imgs, seeds, [int(x) for x in offs], _pcuts(pkg, cuts))
    torch.cuda.synchronize()
    assert torch.equal(res["tree"], tree)
    check("B", res["planes"], res["lakes"], res["region_stats"], res["offsets"], res["hidden"], res["hidden_stats"])


# ---- (B): cube in, everything out ---------------------------------------------------------------------------------------------------

def _cube_call(pkg, torch, eng, cube, cuts, **kw):
    dcube, seeds, offs, wt = _engine_inputs(torch, eng, cube)
    res = eng.merge_tree_cut_catalogue_batch(dcube, seeds, offs, _pcuts(pkg, cuts), weights=wt, edge=cube.edge, **kw)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("name", bc.STACKING + bc.LOOPING)
def test_cube_form_against_reference(pkg, torch, eng, name):
    cube = bc.cube(name)
    cuts = cube.cuts
    res = _cube_call(pkg, torch, eng, cube, cuts, want_labels=True, want_keys=True)
    assert (_u32(res["tree"]) == cube.tree()).all(), name
    stats, first = ls.from_raw(res["stats"].cpu().numpy()), cube.first_records()
    for k, f in enumerate(cube.slices):      # (a slice without seeds owns the record of its whole plane)
        _same((name, "catalogue", k), stats[first[k]:first[k + 1]], f.stats if f.n_seeds else bc.cc.whole_plane(f).reshape(1))
    assert (_u32(res["labels"]) == cube.seg()).all(), name
    _check(name, cube, cuts, res["planes"], res["lakes"], res["region_stats"], res["offsets"], res["hidden"], res["hidden_stats"])
    # the stamps it hands back are every slice's own: ws_copy_last_arrival_device after ws_merge_tree_device on the slice alone
    dcube, seeds, offs, wt = _engine_inputs(torch, eng, cube)
    for k in range(cube.n_slices):
        if cube.slices[k].n_seeds == 0:
            continue
        eng.merge_tree(dcube[k], seeds[offs[k]:offs[k + 1]], edge=cube.edge)
        assert torch.equal(eng.last_arrival(), res["keys"][k]), (name, k)
    # ... and with the labels they feed (A) in a second call, which yields the same outputs
    pw = _dev(torch, eng, cube.plane_weights())
    again = eng.tree_cut_catalogue_batch(res["tree"], res["keys"], res["labels"], offs, _pcuts(pkg, cuts), weights=pw, stats=res["stats"])
    torch.cuda.synchronize()
    assert torch.equal(again[0], res["planes"]) and torch.equal(again[1], res["lakes"]) and torch.equal(again[2], res["region_stats"])
    assert (again[3] == res["offsets"]).all() and (again[4] == res["hidden"]).all() and (again[5] == res["hidden_stats"]).all()
    # the per-slice views are the single call's tuples
    for k, view in enumerate(res["slices"]):
        p = cube.expected(cuts)[k]
        assert (np.asarray(view[3]) == p[3]).all() and (view[1].cpu().numpy().view(np.uint64) == p[1]).all(), (name, k)
    # without the catalogue (no statistics pass) the cuts by area, leaves and level are the same
    plain = [c for c in cuts if not c.catalogue]
    res2 = _cube_call(pkg, torch, eng, cube, plain, want_stats=False)
    assert res2["stats"] is None and torch.equal(res2["tree"], res["tree"])
    _check((name, "no stats"), cube, plain, res2["planes"], res2["lakes"], res2["region_stats"], res2["offsets"], res2["hidden"], res2["hidden_stats"])


def test_cube_form_in_groups_and_capacity(pkg, torch, eng):
    """Five slices as groups of 2, 2 and 1 (a seedless slice inside the first): lists cross group boundaries; cap one short in the
    last group and in the first: *n_lakes is the need and the region records are untouched from the overflow on."""
    cube = bc.cube("5x40x96")
    cuts = cube.cuts
    h, w = cube.plane_shape
    whole = _cube_call(pkg, torch, eng, cube, cuts)
    eng.ctx.set_batch_pixel_limit(2 * h * w)
    try:
        res = _cube_call(pkg, torch, eng, cube, cuts)
        _check("groups", cube, cuts, res["planes"], res["lakes"], res["region_stats"], res["offsets"], res["hidden"], res["hidden_stats"])
        assert torch.equal(res["lakes"], whole["lakes"]) and torch.equal(res["region_stats"], whole["region_stats"])
        need = len(cube.expected_flat(cuts)[0])
        k = len(cuts)
        group_ends = [int(res["offsets"][2 * k]), int(res["offsets"][4 * k]), need]
        assert 0 < group_ends[0] < group_ends[1] < need
        dcube, seeds, offs, wt = _engine_inputs(torch, eng, cube)
        s = cube.n_slices
        for cap, written in ((need - 1, group_ends[1]), (group_ends[0] - 1, 0)):
            lakes = torch.full((need, 2), -1, dtype=torch.int64, device=eng.device)
            region = torch.full((need, 9), -1, dtype=torch.int64, device=eng.device)
            tree = torch.empty((offs[-1] + s, 4), dtype=torch.int32, device=eng.device)
            stats = torch.empty((offs[-1] + s, 9), dtype=torch.int64, device=eng.device)
            offsets, hidden, hs = np.zeros(s * k + 1, np.uint64), np.zeros(s * k, np.uint64), np.zeros((s * k, 9), np.int64)
            n, failed = ctypes.c_size_t(0), ctypes.c_size_t(0)
            opt = eng.options(254, False, None, False)
            rc = pkg._ffi.lib().ws_merge_tree_cut_catalogue_batch_device(
                eng.ctx.handle, dcube.data_ptr(), s, h, w, w, h * w, seeds.data_ptr(), (ctypes.c_size_t * (s + 1))(*offs), ctypes.byref(opt),
                wt.data_ptr(), pkg._ffi.WS_DTYPES["uint16"], w, h * w, _lake_cuts(pkg, cuts), k, tree.data_ptr(), stats.data_ptr(), None, None, None, 0,
                lakes.data_ptr(), region.data_ptr(), cap, ctypes.byref(n), offsets.ctypes.data, hidden.ctypes.data, hs.ctypes.data,
                ctypes.byref(failed))
            torch.cuda.synchronize()
            assert rc == pkg._ffi.WS_ERR_CAPACITY and n.value == need, (rc, n.value, need)
            assert (region[written:] == -1).all() and (lakes[written:] == -1).all(), cap
            assert torch.equal(tree, whole["tree"])      # the remaining groups still flooded
    finally:
        eng.ctx.set_batch_pixel_limit(0)


def test_abandoned_stack_gives_the_loops_results(pkg, torch, eng):
    """The last slice's seed list is reversed: its group mispredicts after two groups have written, the stack is abandoned and
    the loop starts over from record 0 (tests/test_gpu_batch_fallback.py's way to leave the stack)."""
    src = bc.cube("5x40x96")
    lists = [l.copy() for l in src.lists]
    lists[4] = lists[4][::-1].copy()
    cube = bc.Cube("reversed", src.imgs, lists, src.weights, False, src.cuts)
    h, w = cube.plane_shape
    eng.ctx.set_batch_pixel_limit(2 * h * w)
    try:
        res = _cube_call(pkg, torch, eng, cube, cube.cuts, want_labels=True)
    finally:
        eng.ctx.set_batch_pixel_limit(0)
    assert (_u32(res["tree"]) == cube.tree()).all() and (_u32(res["labels"]) == cube.seg()).all()
    _check("reversed", cube, cube.cuts, res["planes"], res["lakes"], res["region_stats"], res["offsets"], res["hidden"], res["hidden_stats"])


# ---- refusals: every output prefilled and found untouched -----------------------------------------------------------------------------

def _raw_a(pkg, eng, torch, cube, cuts, tree=None, stats="own", offs=None, keys=None, labels=None, weights="own", wrow=None, wslice=None, stride=None,
           out="own", lakes="own", region="own", n_cuts=None):
    """ws_tree_cut_catalogue_batch_device as it stands with prefilled outputs; returns (rc, every output untouched)."""
    s, (h, w), k = cube.n_slices, cube.plane_shape, len(cuts) if n_cuts is None else n_cuts
    t0, st0, k0, l0, w0 = _oracle_inputs(torch, eng, cube)
    tree = t0 if tree is None else tree
    keys = k0 if keys is None else keys
    labels = l0 if labels is None else labels
    stats = st0 if isinstance(stats, str) else stats
    wt = w0 if isinstance(weights, str) else weights
    planes = torch.full((s * max(k, 1) * h * w,), S32, dtype=torch.int32, device=eng.device)
    out_p = planes.data_ptr() if isinstance(out, str) else out
    lk = torch.full((4096, 2), -1, dtype=torch.int64, device=eng.device)
    rg = torch.full((4096, 9), -1, dtype=torch.int64, device=eng.device)
    offsets, hidden, hs = np.full(s * max(k, 1) + 1, 77, np.uint64), np.full(s * max(k, 1), 77, np.uint64), np.full((s * max(k, 1), 9), 77, np.int64)
    n = ctypes.c_size_t(77)
    offs = cube.seed_offsets() if offs is None else offs
    dt = pkg._ffi.WS_DTYPES["uint16" if wt is not None and wt.dtype == torch.int16 else "uint8"]
    rc = pkg._ffi.lib().ws_tree_cut_catalogue_batch_device(
        eng.ctx.handle, tree.data_ptr(), stats.data_ptr() if stats is not None else None, s, (ctypes.c_size_t * (s + 1))(*offs), keys.data_ptr(),
        labels.data_ptr(), h, w, wt.data_ptr() if wt is not None else None, dt, w if wrow is None else wrow, h * w if wslice is None else wslice,
        _lake_cuts(pkg, cuts), k, out_p, h * w if stride is None else stride, lk.data_ptr() if isinstance(lakes, str) else lakes,
        rg.data_ptr() if isinstance(region, str) else region, 4096, ctypes.byref(n), offsets.ctypes.data, hidden.ctypes.data, hs.ctypes.data)
    torch.cuda.synchronize()
    clean = bool((planes == S32).all()) and bool((lk == -1).all()) and bool((rg == -1).all()) and (offsets == 77).all() and (hidden == 77).all() \
        and (hs == 77).all() and n.value == 77
    return rc, clean, planes


def test_refusals_leave_every_output_untouched(pkg, torch, eng):
    cube = bc.cube("9x8x16")
    cuts = cube.cuts[:4]
    first, offs = cube.first_records(), cube.seed_offsets()
    h, w = cube.plane_shape
    BAD = pkg._ffi.WS_ERR_BAD_ARG
    tree = cube.tree()
    dead = [(k, c) for k in range(cube.n_slices) for c in range(1, cube.slices[k].n_seeds + 1) if tree[first[k] + c, 1] != bc.ALIVE]

    def refused(**kw):
        rc, clean, _ = _raw_a(pkg, eng, torch, cube, kw.pop("cuts", cuts), **kw)
        assert rc == BAD and clean, (kw.keys(), rc, clean, _err(pkg, eng))

    # a record that is a merge-tree record in the single-plane sense of the whole array, but not within its slice
    i, p = bc.foreign_parent(cube)
    t = tree.copy()
    t[i, 0] = p
    refused(tree=_dev(torch, eng, t))
    # a dead record with parent 0 in the last slice only
    k, c = [x for x in dead if x[0] == cube.n_slices - 1][0]
    t = tree.copy()
    t[first[k] + c, 0] = 0
    refused(tree=_dev(torch, eng, t))
    # decreasing offsets
    bad_offs = list(offs)
    bad_offs[3] = bad_offs[2] - 1 if bad_offs[2] else bad_offs[4] + 1
    refused(offs=bad_offs)
    refused(stride=h * w - 1)                              # a short plane_stride
    refused(wslice=h * w - 1)                              # a short weight_slice_stride
    refused(wrow=w - 1)
    bad = _lake_cuts(pkg, cuts)
    rsv = [bc.Cut()] * 33
    refused(cuts=rsv)                                      # 33 cuts
    refused(lakes=None)                                    # d_region_stats without d_lakes
    refused(stats=None, cuts=[bc.Cut(min_depth=3)])        # a catalogue threshold with d_stats == NULL
    k0 = _dev(torch, eng, cube.keys())
    rc = _raw_a(pkg, eng, torch, cube, cuts, keys=k0, out=k0.data_ptr())[0]      # d_out aliasing an input (its words are not prefilled)
    assert rc == BAD and (_u32(k0) == cube.keys()).all()
    # non-zero reserved bytes
    bad[1].reserved[2] = 1
    t0, st0, kk, ll, w0 = _oracle_inputs(torch, eng, cube)
    out = torch.full((cube.n_slices * 4 * h * w,), S32, dtype=torch.int32, device=eng.device)
    rc = pkg._ffi.lib().ws_tree_cut_catalogue_batch_device(
        eng.ctx.handle, t0.data_ptr(), st0.data_ptr(), cube.n_slices, (ctypes.c_size_t * (cube.n_slices + 1))(*offs), kk.data_ptr(), ll.data_ptr(), h, w,
        None, 0, 0, 0, bad, 4, out.data_ptr(), h * w, None, None, 0, None, None, None, None)
    torch.cuda.synchronize()
    assert rc == BAD and (out == S32).all()


def test_label_above_its_own_slices_seed_count_is_written_as_zero_and_reported_late(pkg, torch, eng):
    """Label n_k + 1 in a slice whose successor has more seeds: a valid record index of the next slice, refused by the per-slice bound."""
    cube = bc.cube("9x8x16")
    cuts = cube.cuts[:3]
    ns = [f.n_seeds for f in cube.slices]
    k = [i for i in range(cube.n_slices - 1) if 0 < ns[i] < ns[i + 1]][0]
    seg = cube.seg().copy()
    r, c = np.argwhere((seg[k] != 0) & (cube.keys()[k] >> 24 == 0))[0]      # a seed pixel: shown by every cut
    seg[k, r, c] = ns[k] + 1
    rc, clean, planes = _raw_a(pkg, eng, torch, cube, cuts, labels=_dev(torch, eng, seg))
    assert rc == pkg._ffi.WS_ERR_BAD_ARG and "label" in _err(pkg, eng)
    h, w = cube.plane_shape
    got = _u32(planes).reshape(cube.n_slices, len(cuts), h, w)
    per = cube.expected(cuts)
    for j in range(len(cuts)):
        assert got[k, j, r, c] == 0
        want = per[k][0][j].copy()
        want[r, c] = 0
        assert (got[k, j] == want).all() and (got[k + 1, j] == per[k + 1][0][j]).all()


def test_context_with_a_begun_transform_is_refused(pkg, torch, eng):
    cube = bc.cube("9x8x16")
    img = torch.from_numpy(cube.imgs[0]).to(eng.device)
    seeds = torch.from_numpy(cube.lists[0].astype(np.int32)).to(eng.device)
    labels = torch.empty(cube.plane_shape, dtype=torch.int32, device=eng.device)
    eng.segment_begin(img, seeds, labels)
    try:
        rc, clean, _ = _raw_a(pkg, eng, torch, cube, cube.cuts[:2])
    finally:
        eng.segment_end()
    torch.cuda.synchronize()
    assert rc == pkg._ffi.WS_ERR_BAD_ARG and clean


# ---- the host form and the shim -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["9x8x16", "5x130x98"])
def test_host_form_and_shim(pkg, name):
    cube = bc.cube(name)
    cuts = cube.cuts
    ws = pkg.TransformBuilder.new().build_merging()
    got = ws.merge_tree_cut_catalogue_cube(np.stack(cube.imgs), cube.lists, _pcuts(pkg, cuts), weights=cube.weights, want_tree=True, want_stats=True)
    per = cube.expected(cuts)
    assert len(got) == cube.n_slices
    first = cube.first_records()
    for k, (planes, lakes, region, offsets, hidden, hidden_stats, tree, stats) in enumerate(got):
        want = per[k]
        for j in range(len(cuts)):
            assert planes.dtype == np.uint64 and (planes[j] == want[0][j]).all(), (name, k, j)
        assert (np.asarray(lakes).view(np.uint64).reshape(-1, 2) == want[1]).all() and (offsets == want[3]).all() and (hidden == want[4]).all(), (name, k)
        _same((name, k, "regions"), region, want[2])
        _same((name, k, "hidden"), hidden_stats, want[5])
        t = cube.tree()[first[k]:first[k + 1]]
        assert (tree.parent == t[:, 0]).all() and (tree.death_level == t[:, 1]).all() and (tree.area == t[:, 2]).all(), (name, k)
        if cube.slices[k].n_seeds:
            _same((name, k, "catalogue"), stats, cube.slices[k].stats)
    # seeds=None: every slice's own minima
    own = bc.Cube(name + "_minima", cube.imgs, [bc._minima(im) for im in cube.imgs], cube.weights, False)
    plain = [c for c in cuts if not c.catalogue][:4]
    got = ws.merge_tree_cut_catalogue_cube(np.stack(cube.imgs), None, _pcuts(pkg, plain), weights=cube.weights)
    for k, (planes, lakes, region, offsets, hidden, hidden_stats) in enumerate(got):
        want = own.expected(plain)[k]
        assert all((planes[j] == want[0][j]).all() for j in range(len(plain))) and (np.asarray(lakes).view(np.uint64).reshape(-1, 2) == want[1]).all(), (name, k)
        _same((name, k, "minima regions"), region, want[2])
