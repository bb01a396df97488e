"""merge_tree of a cube of slices in one call (ws_merge_tree_batch(_device)), on the GPU: every slice's records against
ws_merge_tree_device on that slice alone and the tree derived from the CPU oracle's planes (tests/merge_tree_ref.py), the stack's
own guarantees (it is taken, groups, failing slice, graph keys on a shared context) and the host form.  Every comparison is on
integers and exact."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import merge_tree_ref as mt
import oracle_lib as ol
import strided

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def stream(torch):
    with torch.cuda.stream(torch.cuda.Stream(0)):      # a stream of its own: the level loops are captured and replayed
        yield


def _engine(pkg):
    return importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


def _ws(pkg, max_level=254, edge=False, seed_shift=False):
    b = pkg.TransformBuilder.new().set_max_water_lvl(max_level)
    if edge:
        b.enable_edge_correction()
    if seed_shift:
        b.shift_seeds_into_padded_plane()
    return b.build_merging()


def _minima(imgs):
    return [np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2) for im in imgs]


def _seed_lists(imgs):
    """As tests/test_gpu_history_batch.py: the slices' own minima, except: slice 1 has no seed, slice 2 a single one."""
    lists = _minima(imgs)
    lists[1] = lists[1][:0]
    lists[2] = lists[2][:1]
    return lists


def _device_inputs(torch, eng, imgs, lists):
    flat = np.concatenate(lists, axis=0) if sum(len(l) for l in lists) else np.zeros((0, 2), np.int64)
    offs = [0] + [int(x) for x in np.cumsum([len(l) for l in lists])]
    cube = torch.from_numpy(np.stack(imgs)).to(eng.device).contiguous()
    return cube, torch.from_numpy(flat.astype(np.int32)).to(eng.device).contiguous(), offs


def _first(offs):
    """First record of every slice (and the total): slice k's n_k + 1 records start at (offs[k] - offs[0]) + k."""
    return [int(offs[k]) - int(offs[0]) + k for k in range(len(offs))]


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _raw_device(pkg, eng, cube_ptr, shape, seeds_ptr, offs, tree_ptr, labels_ptr=None, max_level=254, edge=False, failed=None,
                row_stride=None, slice_stride=None, opt=None, null_opt=False):
    """ws_merge_tree_batch_device itself."""
    import torch
    s, h, w = shape
    opt = opt if opt is not None else eng.options(max_level, edge)
    c_offs = (ctypes.c_size_t * (s + 1))(*[int(x) for x in offs])
    rs = w if row_stride is None else row_stride
    rc = pkg._ffi.lib().ws_merge_tree_batch_device(eng.ctx.handle, cube_ptr, s, h, w, rs, h * rs if slice_stride is None else slice_stride,
                                                   seeds_ptr, c_offs, None if null_opt else ctypes.byref(opt), tree_ptr, labels_ptr,
                                                   ctypes.byref(failed) if failed is not None else None)
    torch.cuda.synchronize()
    return rc


def _check_against_single_calls(eng, cube, seeds, offs, got, labels=None, **kw):
    """Every slice's records (and labels) against eng.merge_tree on that slice alone; returns the per-slice record arrays."""
    first = _first(offs)
    got = _u32(got)
    assert got.shape == (first[-1], 4)
    out = []
    for k in range(cube.shape[0]):
        one, one_labels = eng.merge_tree(cube[k], seeds[offs[k]:offs[k + 1]], want_labels=True, **kw)
        rec = got[first[k]:first[k + 1]]
        assert rec.shape[0] == offs[k + 1] - offs[k] + 1
        bad = np.flatnonzero((rec != _u32(one)).any(axis=1))
        assert bad.size == 0, (k, bad[:8], rec[bad[:8]], _u32(one)[bad[:8]])
        if labels is not None:
            assert (_u32(labels[k]) == _u32(one_labels)).all(), k
        out.append(rec)
    return out


# the stack: the plane (padded with edge correction) is 128 x 96, or 40 x 96 = 3840 pixels, whose 1024-pixel runs of the own-count
# pass straddle slices; no stack: w' % 4 != 0
SHAPES = [((6, 128, 96), False), ((6, 126, 94), True), ((5, 40, 96), False), ((5, 130, 98), False), ((5, 130, 98), True)]


@pytest.mark.parametrize("max_level", [254, 90])
@pytest.mark.parametrize("shape,edge", SHAPES)
def test_tree_batch_matches_single_calls_and_reference_per_slice(pkg, torch, shape, edge, max_level):
    s, h, w = shape
    eng = _engine(pkg)
    imgs = [cases.field(h, w, 2100 + 7 * k) for k in range(s)]
    lists = _seed_lists(imgs)
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    got, labels = eng.merge_tree_batch(cube, seeds, offs, max_level=max_level, edge=edge, want_labels=True)
    torch.cuda.synchronize()
    e = 2 if edge else 0
    assert tuple(labels.shape) == (s, h + e, w + e)
    assert torch.equal(labels, eng.segment_batch(cube, seeds, offs, max_level=max_level, edge=edge))
    recs = _check_against_single_calls(eng, cube, seeds, offs, got, labels, max_level=max_level, edge=edge)
    lab = _u32(labels)
    for k in range(s):
        parent, death, area, leaves, vals, ex = mt.expected_tree(imgs[k], lists[k], max_level, edge)
        want = np.stack([parent, death, area, leaves], axis=1)
        bad = np.flatnonzero((recs[k] != want).any(axis=1))
        assert bad.size == 0, (shape, edge, max_level, k, bad[:8], recs[k][bad[:8]], want[bad[:8]])
        mt.check_invariants(recs[k][:, 0], recs[k][:, 1], recs[k][:, 2], recs[k][:, 3], vals, ex)
        assert recs[k][0].tolist() == [0, mt.ALIVE, int((lab[k] == 0).sum()), 0], k
    assert recs[1].shape[0] == 1 and recs[2].shape[0] == 2                  # the seedless slice owns its record 0 alone


def test_seed_shift_duplicate_seed_and_saturated_slice(pkg, torch):
    eng = _engine(pkg)
    s, h, w = 5, 126, 94
    imgs = [cases.field(h, w, 2200 + k) for k in range(s)]
    # edge correction with the seeds moved into the padded plane (128 x 96: a stack)
    lists = _seed_lists(imgs)
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    got, labels = eng.merge_tree_batch(cube, seeds, offs, edge=True, seed_shift=True, want_labels=True)
    recs = _check_against_single_calls(eng, cube, seeds, offs, got, labels, edge=True, seed_shift=True)
    want = mt.expected_tree(imgs[3], lists[3], 254, True, True)
    assert (recs[3] == np.stack(want[:4], axis=1)).all()
    # a slice of 255s in a stack; then a duplicated seed in slice 3 as well (the stack mispredicts into the loop; the later
    # colour overwrites)
    s, h, w = 5, 128, 96
    imgs = [cases.field(h, w, 2250 + k) for k in range(s)]
    imgs[4] = np.full((h, w), 255, dtype=np.uint8)
    lists = _minima(imgs)
    lists[4] = np.array([[5, 7], [90, 33]], np.int64)
    for duplicate in (False, True):
        if duplicate:
            lists[3] = np.concatenate([lists[3][:40], lists[3][10:11], lists[3][40:]])
        cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
        got, labels = eng.merge_tree_batch(cube, seeds, offs, want_labels=True)
        recs = _check_against_single_calls(eng, cube, seeds, offs, got, labels)
        assert recs[4][0].tolist() == [0, mt.ALIVE, h * w - 2, 0]                   # nothing floods at 255: the two seed pixels
        assert recs[4][1:].tolist() == [[0, mt.ALIVE, 1, 1], [0, mt.ALIVE, 1, 1]]
    assert recs[3][11].tolist() == [0, mt.ALIVE, 0, 0] and recs[3][41][3] >= 1      # colour 11 never was: colour 41 sits on its pixel
    want = mt.expected_tree(imgs[3], lists[3])
    assert (recs[3] == np.stack(want[:4], axis=1)).all()


def test_only_the_calls_records_are_written_and_refusals_touch_nothing(pkg, torch):
    eng = _engine(pkg)
    L = pkg._ffi.lib()
    BAD = pkg._ffi.WS_ERR_BAD_ARG
    for shape in ((4, 128, 96), (4, 130, 98)):
        s, h, w = shape
        imgs = [cases.field(h, w, 2300 + k) for k in range(s)]
        lists = _seed_lists(imgs)
        cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
        total = _first(offs)[-1]
        tree = torch.full((total + 64, 4), SENTINEL, dtype=torch.int32, device=eng.device)
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs, tree.data_ptr()) == 0
        assert bool((tree[total:] == SENTINEL).all())
        _check_against_single_calls(eng, cube, seeds, offs, tree[:total])
        # offsets that do not start at 0: the records still start at the front of d_tree
        tree.fill_(SENTINEL)
        shifted = [o + 5 for o in offs]
        pad = torch.cat([torch.zeros((5, 2), dtype=torch.int32, device=eng.device), seeds]).contiguous()
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, pad.data_ptr(), shifted, tree.data_ptr()) == 0
        assert bool((tree[total:] == SENTINEL).all())
        _check_against_single_calls(eng, cube, seeds, offs, tree[:total])
        # refused calls
        tree.fill_(SENTINEL)
        labels = torch.full((s, h, w), SENTINEL, dtype=torch.int32, device=eng.device)
        args = (pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs, tree.data_ptr(), labels.data_ptr())
        assert _raw_device(pkg, eng, None, shape, seeds.data_ptr(), offs, tree.data_ptr(), labels.data_ptr()) == BAD
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, None, offs, tree.data_ptr(), labels.data_ptr()) == BAD
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs, None, labels.data_ptr()) == BAD
        assert _raw_device(*args, null_opt=True) == BAD
        assert _raw_device(*args, row_stride=w - 1) == BAD
        assert _raw_device(*args, slice_stride=h * w - 1) == BAD
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs[:2] + [offs[1] - 1] + offs[3:], tree.data_ptr()) == BAD
        assert _raw_device(*args, opt=eng.options(max_level=255)) == pkg._ffi.WS_ERR_MAX_TOO_HIGH
        assert _raw_device(*args, opt=eng.options(max_level=0)) == pkg._ffi.WS_ERR_MAX_TOO_LOW
        out = torch.empty((h, w), dtype=torch.int32, device=eng.device)
        eng.segment_begin(cube[0], seeds[offs[0]:offs[1]], out)      # a transform in flight is refused
        try:
            assert _raw_device(*args) == BAD
        finally:
            eng.segment_end()
        torch.cuda.synchronize()
        assert bool((tree == SENTINEL).all()) and bool((labels == SENTINEL).all())
        # no slice: nothing is written
        assert _raw_device(pkg, eng, None, (0, h, w), None, [0], None) == 0
        assert tuple(eng.merge_tree_batch(cube[:0], seeds[:0], [0]).shape) == (0, 4)


def test_stack_is_taken_at_size(pkg, torch):
    s, h, w = 16, 1024, 1024
    eng = _engine(pkg)
    cube = torch.stack([eng.random_field(h, w, 2400 + k) for k in range(s)]).contiguous()
    lists = [eng.find_local_minima(cube[k]) for k in range(s)]
    offs = [0] + [int(x) for x in np.cumsum([int(l.shape[0]) for l in lists])]
    seeds = torch.cat(lists).contiguous()
    got = eng.merge_tree_batch(cube, seeds, offs)
    batch_relax = eng.stats()["launches_relax"]
    first = _first(offs)
    loop_relax = 0
    for k in range(s):
        one = eng.merge_tree(cube[k], lists[k])
        loop_relax += eng.stats()["launches_relax"]
        rec = got[first[k]:first[k + 1]]
        assert torch.equal(rec, one), k
        alive = (rec[:, 1] == -1) & (rec[:, 3] > 0)
        alive[0] = False
        assert int(rec[alive, 2].to(torch.int64).sum()) + int(rec[0, 2]) == h * w, k
    assert batch_relax < loop_relax, (batch_relax, loop_relax)      # one stacked flood, not sixteen


def test_several_groups_equal_one(pkg, torch):
    s, h, w = 7, 128, 96
    eng = _engine(pkg)
    imgs = [cases.field(h, w, 2500 + k) for k in range(s)]
    lists = _minima(imgs)
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    one_group, one_labels = eng.merge_tree_batch(cube, seeds, offs, want_labels=True)
    one_relax = eng.stats()["launches_relax"]
    eng.ctx.set_batch_pixel_limit(3 * h * w)                        # 3 + 3 + 1 slices
    try:
        groups, labels = eng.merge_tree_batch(cube, seeds, offs, want_labels=True)
        groups_relax = eng.stats()["launches_relax"]
    finally:
        eng.ctx.set_batch_pixel_limit(0)
    assert torch.equal(groups, one_group) and torch.equal(labels, one_labels)
    assert groups_relax > one_relax                                 # three floods, not one
    _check_against_single_calls(eng, cube, seeds, offs, groups, labels)


@pytest.mark.parametrize("shape", [(6, 128, 96), (5, 130, 98)])
def test_failing_slice_is_named(pkg, torch, shape):
    s, h, w = shape
    eng = _engine(pkg)
    imgs = [cases.field(h, w, 2600 + k) for k in range(s)]
    for bad_k in (3, 0):
        lists = _minima(imgs)
        lists[bad_k] = np.concatenate([lists[bad_k], np.array([[4000, 3]], np.int64)])
        cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
        tree = torch.empty((_first(offs)[-1], 4), dtype=torch.int32, device=eng.device)
        failed = ctypes.c_size_t(99)
        rc = _raw_device(pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs, tree.data_ptr(), failed=failed)
        assert rc == pkg._ffi.WS_ERR_SEED_OOB and failed.value == bad_k, (shape, bad_k, rc, failed.value)
    # ... and the context works on
    lists = _minima(imgs)
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    recs = _check_against_single_calls(eng, cube, seeds, offs, eng.merge_tree_batch(cube, seeds, offs))
    assert (recs[s - 1] == np.stack(mt.expected_tree(imgs[s - 1], lists[s - 1])[:4], axis=1)).all()


def test_tree_history_list_single_and_merge_batches_alternate_on_one_context(pkg, torch, stream):
    # merge_host captures its level loop on the second of two calls with the same key in a row and replays it from then on.  The
    # stacked tree loop's graphs are those of the stacked history loop; every other kind of call has its own.  On ONE context, each
    # of five kinds of call in turn, three rounds of three calls: a graph replayed for the wrong kind would leave the forest
    # unstamped, or stamp it in another numbering, and a record, a plane or a label would change.
    eng = _engine(pkg)
    L = pkg._ffi.lib()
    s, h, w = 4, 128, 96
    imgs = [cases.field(h, w, 2700 + k) for k in range(s)]
    lists = _minima(imgs)
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    levels = [254, 0, 77, 160, 121]
    first = {}

    def tree_batch():
        return eng.merge_tree_batch(cube, seeds, offs).clone()

    def history_batch():
        return eng.transform_history_batch(cube, seeds, offs, levels=levels, merging=True).clone()

    def list_batch():      # (records within a (slice, level) come in no particular order: compared as sorted keys)
        lakes, offsets, unc = eng.transform_to_list_batch(cube, seeds, offs, merging=True)
        counts = torch.from_numpy(np.diff(offsets.astype(np.int64))).to(lakes.device)
        b = torch.repeat_interleave(torch.arange(counts.numel(), device=lakes.device, dtype=torch.int64), counts)
        return torch.sort((b << 40) | (lakes[:, 0] << 20) | lakes[:, 1]).values, offsets.copy(), unc.copy()

    def single_tree():
        return eng.merge_tree(cube[2], seeds[offs[2]:offs[3]]).clone()

    def merge_batch():
        return eng.merge_batch(cube, seeds, offs).clone()

    def same(a, b):
        if isinstance(a, tuple):
            return torch.equal(a[0], b[0]) and (a[1] == b[1]).all() and (a[2] == b[2]).all()
        return torch.equal(a, b)

    want = np.concatenate([np.stack(mt.expected_tree(imgs[k], lists[k])[:4], axis=1) for k in range(s)])
    for rep in range(3):
        for fn in (tree_batch, history_batch, list_batch, single_tree, merge_batch):
            for i in range(3):
                got = fn()
                torch.cuda.synchronize()
                if fn.__name__ not in first:
                    first[fn.__name__] = got
                assert same(got, first[fn.__name__]), (rep, fn.__name__, i)
                if fn is tree_batch:
                    assert (_u32(got) == want).all(), (rep, i)
                    if i == 2:      # captured by the second call, replayed by the third: every group of 16 levels a graph launch
                        assert eng.stats()["graph_launches"] >= 16, (rep, eng.stats()["graph_launches"])
                    p = ctypes.c_void_p()
                    hh, ww = ctypes.c_size_t(), ctypes.c_size_t()
                    assert L.ws_last_arrival_device(eng.ctx.handle, ctypes.byref(p), ctypes.byref(hh), ctypes.byref(ww)) == \
                        pkg._ffi.WS_ERR_UNSUPPORTED
    first_rec = _first(offs)
    assert (_u32(first["single_tree"]) == want[first_rec[2]:first_rec[3]]).all()


def _rows(t):
    return np.stack([t.parent, t.death_level, t.area, t.n_leaves], axis=1)


@pytest.mark.parametrize("shape", [(5, 128, 112), (5, 130, 98)])      # a stack, and the loop
def test_host_form_equals_slice_calls(pkg, shape):
    s, h, w = shape
    cube = np.stack([cases.field(h, w, 2800 + k) for k in range(s)])
    ws = _ws(pkg, max_level=200)
    mins = [ws.find_local_minima(cube[k]) for k in range(s)]
    got, counts = ws.merge_tree_cube(cube, want_labels=True)
    lists = list(mins)
    lists[1] = lists[1][:0]
    lists[2] = lists[2][:1]
    given = ws.merge_tree_cube(cube, seeds=lists)
    assert len(got) == len(given) == s
    for k in range(s):
        assert counts[k] == len(mins[k])
        want = ws.merge_tree(cube[k], mins[k], want_labels=True)
        assert (_rows(got[k]) == _rows(want)).all(), k
        assert got[k].labels.dtype == np.uint64 and (got[k].labels == want.labels).all(), k
        assert given[k].labels is None and (_rows(given[k]) == _rows(ws.merge_tree(cube[k], lists[k]))).all(), k
    # the raw call with room for one record less: the count, and nothing else
    L = pkg._ffi.lib()
    total = int(sum(counts)) + s
    tree = np.full((total, 4), SENTINEL, dtype=np.uint32)
    labels = np.full((s, h, w), SENTINEL, dtype=np.uint64)
    n_rec, failed = ctypes.c_size_t(0), ctypes.c_size_t(0)
    n_seeds = np.zeros(s, dtype=np.uintp)
    ctx = ws._ctx()
    args = (ctx.handle, cube.ctypes.data, s, h, w, w, h * w, None, None, ctypes.byref(ws._opt), tree.ctypes.data)
    tail = (ctypes.byref(n_rec), labels.ctypes.data, n_seeds.ctypes.data_as(pkg._ffi.szp), ctypes.byref(failed))
    assert L.ws_merge_tree_batch(*args, total - 1, *tail) == pkg._ffi.WS_ERR_CAPACITY
    assert n_rec.value == total and (n_seeds == counts).all()
    assert (tree == SENTINEL).all() and (labels == SENTINEL).all()
    assert L.ws_merge_tree_batch(*args, total, *tail) == 0
    assert n_rec.value == total and (tree == np.concatenate([_rows(t) for t in got])).all()
    assert (labels == np.stack([t.labels for t in got])).all()


@pytest.mark.parametrize("shape,edge", [((4, 128, 96), False), ((4, 75, 101), True)])
def test_strided_cube(pkg, torch, shape, edge):
    s, h, w = shape
    eng = _engine(pkg)
    imgs = [cases.field(h, w, 2900 + k) for k in range(s)]
    lists = _seed_lists(imgs)
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    want, want_labels = eng.merge_tree_batch(cube, seeds, offs, edge=edge, want_labels=True)
    rs = w + 5
    ss = h * rs + 77
    backing, off, _ = strided.embed_cube(np.stack(imgs), 3, rs, ss, 0x00)
    t_back = torch.from_numpy(backing).to(eng.device)
    e = 2 if edge else 0
    tree = torch.full((want.shape[0] + 8, 4), SENTINEL, dtype=torch.int32, device=eng.device)
    labels = torch.empty((s, h + e, w + e), dtype=torch.int32, device=eng.device)
    rc = _raw_device(pkg, eng, t_back.data_ptr() + off, shape, seeds.data_ptr(), offs, tree.data_ptr(), labels.data_ptr(), edge=edge,
                     row_stride=rs, slice_stride=ss)
    assert rc == 0
    assert torch.equal(tree[:want.shape[0]], want) and bool((tree[want.shape[0]:] == SENTINEL).all())
    assert torch.equal(labels, want_labels)
    host = _ws(pkg, edge=edge).merge_tree_cube(strided.view_cube(backing, off, s, h, w, rs, ss), seeds=[l.astype(np.uint64) for l in lists])
    assert (np.concatenate([_rows(t) for t in host]) == _u32(want)).all()


def test_torch_mirror_equals_host_form_and_reuses_out(pkg, torch):
    eng = _engine(pkg)
    s, h, w = 4, 126, 94
    imgs = [cases.smooth_field(h, w, 3000 + k) for k in range(s)]
    lists = _minima(imgs)
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    total = _first(offs)[-1]
    out = torch.full((total, 4), -7, dtype=torch.int32, device=eng.device)
    got, labels = eng.merge_tree_batch(cube, seeds, offs, edge=True, want_labels=True, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (total, 4) and got.dtype == torch.int32
    again = eng.merge_tree_batch(cube, seeds, offs, edge=True, out=out)
    assert again.data_ptr() == out.data_ptr()
    host = _ws(pkg, edge=True).merge_tree_cube(np.stack(imgs), seeds=[l.astype(np.uint64) for l in lists], want_labels=True)
    assert (np.concatenate([_rows(t) for t in host]) == _u32(got)).all()
    assert (np.stack([t.labels for t in host]) == _u32(labels).astype(np.uint64)).all()
    with pytest.raises(ValueError):
        eng.merge_tree_batch(cube, seeds, offs, out=torch.empty((total + 1, 4), dtype=torch.int32, device=eng.device))


def test_roots_tables_give_the_history_planes_at_size(pkg, torch):
    s, h, w = 8, 512, 512
    eng = _engine(pkg)
    cube = torch.stack([eng.random_field(h, w, 3100 + k) for k in range(s)]).contiguous()
    lists = [eng.find_local_minima(cube[k]) for k in range(s)]
    offs = [0] + [int(x) for x in np.cumsum([int(l.shape[0]) for l in lists])]
    seeds = torch.cat(lists).contiguous()
    levels = [118, 201]
    tree, labels = eng.merge_tree_batch(cube, seeds, offs, want_labels=True)
    planes = _u32(eng.transform_history_batch(cube, seeds, offs, levels=levels, merging=True))
    rec, lab, first = _u32(tree), _u32(labels), _first(offs)
    for k in range(s):
        r = rec[first[k]:first[k + 1]]
        t = pkg.MergeTree(r[:, 0], r[:, 1], r[:, 2], r[:, 3])
        for j, lvl in enumerate(levels):
            shown = planes[k, j] != 0
            assert shown.any() and (t.roots_at(lvl)[lab[k]][shown] == planes[k, j][shown]).all(), (k, lvl)
