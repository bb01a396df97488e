"""merge_tree_stats of a cube of slices in one call (ws_merge_tree_stats_batch(_device)), on the GPU.  The yardsticks are never the
batch itself: every slice's records against ws_merge_tree_stats_device on that slice alone with that slice's weight plane and
against the records derived from the CPU oracle's planes (tests/lake_stats_ref.py), the tree against ws_merge_tree_batch_device,
and closed forms where the image is 255 everywhere.  Every comparison is on integers and exact."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import lake_stats_batch_cases as bc
import lake_stats_ref as ls
import merge_tree_ref as mt
import oracle_lib as ol
import strided

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
SENTINEL64 = 0x5A5A5A5A5A5A5A5A


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


def _engine(pkg):
    return importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


def _ws(pkg, max_level=254, edge=False, seed_shift=False):
    b = pkg.TransformBuilder.new().set_max_water_lvl(max_level)
    if edge:
        b.enable_edge_correction()
    if seed_shift:
        b.shift_seeds_into_padded_plane()
    return b.build_merging()


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


def _rec(t):
    return ls.from_raw(t.cpu().numpy())


def _wt_dev(torch, eng, wt):
    """A u8 cube (or plane) as it is, a u16 one as its int16 bits; None stays None."""
    if wt is None:
        return None
    wt = np.ascontiguousarray(wt)
    return torch.from_numpy(wt if wt.dtype == np.uint8 else wt.view(np.int16)).to(eng.device)


def _check_slices_against_single_calls(torch, eng, cube, seeds, offs, wt, tree, stats, labels=None, **kw):
    """Every slice's tree, records (and labels) against eng.merge_tree_stats on that slice alone with its own weight plane; returns
    the per-slice (tree rows, records)."""
    first = _first(offs)
    tree, stats = _u32(tree), _rec(stats)
    assert tree.shape == (first[-1], 4) and stats.shape == (first[-1],)
    out = []
    for k in range(cube.shape[0]):
        one = eng.merge_tree_stats(cube[k], seeds[offs[k]:offs[k + 1]], weights=_wt_dev(torch, eng, None if wt is None else wt[k]),
                                   want_labels=True, **kw)
        torch.cuda.synchronize()
        t, r = tree[first[k]:first[k + 1]], stats[first[k]:first[k + 1]]
        assert t.shape[0] == offs[k + 1] - offs[k] + 1
        assert (t == _u32(one[0])).all(), k
        assert ls.mismatch(r, _rec(one[1])) is None, (k, ls.mismatch(r, _rec(one[1])))
        if labels is not None:
            assert (_u32(labels[k]) == _u32(one[2])).all(), k
        out.append((t, r))
    return out


@pytest.mark.parametrize("max_level", [254, 90])
@pytest.mark.parametrize("shape,edge", bc.SHAPES)
def test_batch_matches_single_calls_and_reference_per_slice(pkg, torch, shape, edge, max_level):
    s, h, w = shape
    eng = _engine(pkg)
    imgs = bc.random_images(shape)
    lists = bc.seed_lists(imgs)
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    want_tree, want_labels = eng.merge_tree_batch(cube, seeds, offs, max_level=max_level, edge=edge, want_labels=True)
    want_tree, want_labels = want_tree.clone(), want_labels.clone()
    oracle = [mt.oracle_planes(imgs[k], lists[k], max_level, edge) for k in range(s)]
    trees = [mt.tree_from_planes(planes, ps) for planes, ps in oracle]
    for name, wt in bc.weight_cubes(shape, 40):
        tree, stats, labels = eng.merge_tree_stats_batch(cube, seeds, offs, weights=_wt_dev(torch, eng, wt), max_level=max_level, edge=edge,
                                                         want_labels=True)
        torch.cuda.synchronize()
        assert torch.equal(tree, want_tree) and torch.equal(labels, want_labels), name
        got = _check_slices_against_single_calls(torch, eng, cube, seeds, offs, wt, tree, stats, labels, max_level=max_level, edge=edge)
        for k in range(s):
            planes, ps = oracle[k]
            parent, death, area, leaves, vals, ex = trees[k]
            assert (got[k][0] == np.stack([parent, death, area, leaves], axis=1)).all(), (name, k)
            want = ls.stats_from_planes(planes, ps, ls.plane_weights(imgs[k], None if wt is None else wt[k], edge), death, ex)
            assert ls.mismatch(got[k][1], want) is None, (shape, edge, max_level, name, k, ls.mismatch(got[k][1], want))
        assert got[1][1].shape == (1,) and got[2][1].shape == (2,)      # the seedless slice owns its record 0 alone


@pytest.mark.parametrize("case", ["last_rows", "checkerboard"])
def test_uncoloured_pixels_stay_in_their_slice(pkg, torch, case):
    """The image is 255 everywhere: nothing floods, every seed stays its own pixel and every other pixel of a slice is
    uncoloured -- its slice's record 0, and no other slice's, though a workgroup's 1024-pixel step holds uncoloured pixels of two
    slices (tests/test_lake_stats_batch_cpu.py proves that of these inputs).  checkerboard: 1024 seeds a slice, 513 keys a
    workgroup, the table-overflow path."""
    eng = _engine(pkg)
    shape, lists = bc.all_255_case(case)
    s, h, w = shape
    imgs = [np.full((h, w), 255, dtype=np.uint8) for _ in range(s)]
    wt = bc.weight_cubes(shape, 77)[2][1]
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    tree, stats = eng.merge_tree_stats_batch(cube, seeds, offs, weights=_wt_dev(torch, eng, wt))
    torch.cuda.synchronize()
    tree, stats, first = _u32(tree), _rec(stats), _first(offs)
    for k in range(s):
        want = bc.all_255_expected(wt[k], lists[k])
        got = stats[first[k]:first[k + 1]]
        assert ls.mismatch(got, want) is None, (case, k, ls.mismatch(got, want))
        assert (got["peak_pixel"] < h * w).all(), k                      # slice-local
        t = tree[first[k]:first[k + 1]]
        assert t[0].tolist() == [0, mt.ALIVE, h * w - len(lists[k]), 0] and (t[1:, 2] == 1).all()
    _check_slices_against_single_calls(torch, eng, cube, seeds, offs, wt, *eng.merge_tree_stats_batch(cube, seeds, offs, weights=_wt_dev(torch, eng, wt)))


def test_seed_shift_duplicate_seed_level_zero_death_and_empty_record_zero(pkg, torch):
    eng = _engine(pkg)
    # seed shift with edge correction (126 x 94 pads to 128 x 96: a stack)
    shape = (5, 126, 94)
    imgs = bc.random_images(shape, 4300)
    lists = bc.seed_lists(imgs)
    wt = bc.weight_cubes(shape, 43)[2][1]
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    tree, stats, labels = eng.merge_tree_stats_batch(cube, seeds, offs, weights=_wt_dev(torch, eng, wt), edge=True, seed_shift=True, want_labels=True)
    got = _check_slices_against_single_calls(torch, eng, cube, seeds, offs, wt, tree, stats, labels, edge=True, seed_shift=True)
    want_tree, want = ls.expected(imgs[3], lists[3], wt[3], 254, True, True)
    assert (got[3][0] == want_tree).all() and ls.mismatch(got[3][1], want) is None
    # a duplicated seed in slice 3: the later colour exists, the earlier does not
    shape = (5, 128, 96)
    imgs = bc.random_images(shape, 4400)
    lists = [np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2) for im in imgs]
    lists[3] = np.concatenate([lists[3][:40], lists[3][10:11], lists[3][40:]])
    wt = bc.weight_cubes(shape, 44)[2][1]
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    tree, stats = eng.merge_tree_stats_batch(cube, seeds, offs, weights=_wt_dev(torch, eng, wt))
    got = _check_slices_against_single_calls(torch, eng, cube, seeds, offs, wt, tree, stats)
    assert got[3][0][11].tolist() == [0, mt.ALIVE, 0, 0] and got[3][0][41][3] >= 1
    assert got[3][1][11] == ls.empty_records(1)[0]
    want_tree, want = ls.expected(imgs[3], lists[3], wt[3])
    assert (got[3][0] == want_tree).all() and ls.mismatch(got[3][1], want) is None
    # a colour that dies at level 0 in slices 1 and 3: its record is its seed pixel, looked up in the stacked seed pairs
    imgs, lists, dying = bc.level_zero_death_case()
    shape = (len(imgs),) + imgs[0].shape
    for name, wt in bc.weight_cubes(shape, 45):
        for edge, shift in ((False, False), (True, True)):
            cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
            tree, stats = eng.merge_tree_stats_batch(cube, seeds, offs, weights=_wt_dev(torch, eng, wt), edge=edge, seed_shift=shift)
            got = _check_slices_against_single_calls(torch, eng, cube, seeds, offs, wt, tree, stats, edge=edge, seed_shift=shift)
            for k, c in dying:
                want_tree, want = ls.expected(imgs[k], lists[k], None if wt is None else wt[k], 254, edge, shift)
                assert want_tree[c][1] == 0 and want_tree[c][3] == 1
                assert (got[k][0] == want_tree).all() and ls.mismatch(got[k][1], want) is None, (name, edge, k)
                r, x = (int(v) + (1 if edge else 0) for v in lists[k][c - 1])
                v = ls.plane_weights(imgs[k], None if wt is None else wt[k], edge)
                assert got[k][1][c] == ls.pixel_record(v, r, x)
    # a slice with no uncoloured pixel between two that have some: its record 0 is the identity
    imgs, lists, full = bc.empty_record_zero_case()
    shape = (len(imgs),) + imgs[0].shape
    wt = bc.weight_cubes(shape, 46)[2][1]
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    tree, stats = eng.merge_tree_stats_batch(cube, seeds, offs, weights=_wt_dev(torch, eng, wt))
    got = _check_slices_against_single_calls(torch, eng, cube, seeds, offs, wt, tree, stats)
    for k in range(len(imgs)):
        want_tree, want = ls.expected(imgs[k], lists[k], wt[k])
        assert (got[k][0] == want_tree).all() and ls.mismatch(got[k][1], want) is None, k
        assert (got[k][1][0] == ls.empty_records(1)[0]) == (k == full), k


def _raw_device(pkg, eng, cube_ptr, shape, seeds_ptr, offs, tree_ptr, stats_ptr, labels_ptr=None, weight_ptr=None, dtype=0, wrow=None,
                wslice=None, max_level=254, edge=False, failed=None, row_stride=None, slice_stride=None, opt=None, null_opt=False):
    """ws_merge_tree_stats_batch_device itself."""
    import torch
    s, h, w = shape
    opt = opt if opt is not None else eng.options(max_level, edge)
    c_offs = (ctypes.c_size_t * (len(offs)))(*[int(x) for x in offs])
    rs = w if row_stride is None else row_stride
    wr = w if wrow is None else wrow
    rc = pkg._ffi.lib().ws_merge_tree_stats_batch_device(eng.ctx.handle, cube_ptr, s, h, w, rs, h * rs if slice_stride is None else slice_stride,
                                                         seeds_ptr, c_offs, None if null_opt else ctypes.byref(opt), weight_ptr, dtype, wr,
                                                         h * wr if wslice is None else wslice, tree_ptr, stats_ptr, labels_ptr,
                                                         ctypes.byref(failed) if failed is not None else None)
    torch.cuda.synchronize()
    return rc


def test_only_the_calls_records_are_written_and_refusals_touch_nothing(pkg, torch):
    eng = _engine(pkg)
    F = pkg._ffi
    BAD = F.WS_ERR_BAD_ARG
    U16 = F.WS_DTYPES["uint16"]
    for shape in ((4, 128, 96), (4, 130, 98)):
        s, h, w = shape
        imgs = bc.random_images(shape, 4500)
        lists = bc.seed_lists(imgs)
        wt = bc.weight_cubes(shape, 47)[2][1]
        cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
        d_wt = _wt_dev(torch, eng, wt)
        total = _first(offs)[-1]
        tree = torch.full((total + 64, 4), SENTINEL, dtype=torch.int32, device=eng.device)
        stats = torch.full((total + 64, 9), SENTINEL64, dtype=torch.int64, device=eng.device)
        args = (pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs, tree.data_ptr(), stats.data_ptr())
        assert _raw_device(*args, weight_ptr=d_wt.data_ptr(), dtype=U16) == 0
        assert bool((tree[total:] == SENTINEL).all()) and bool((stats[total:] == SENTINEL64).all())
        _check_slices_against_single_calls(torch, eng, cube, seeds, offs, wt, tree[:total], stats[:total])
        # offsets that do not start at 0: the records still start at the front of both arrays
        tree.fill_(SENTINEL)
        stats.fill_(SENTINEL64)
        shifted = [o + 5 for o in offs]
        pad = torch.cat([torch.zeros((5, 2), dtype=torch.int32, device=eng.device), seeds]).contiguous()
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, pad.data_ptr(), shifted, tree.data_ptr(), stats.data_ptr(),
                           weight_ptr=d_wt.data_ptr(), dtype=U16) == 0
        assert bool((tree[total:] == SENTINEL).all()) and bool((stats[total:] == SENTINEL64).all())
        _check_slices_against_single_calls(torch, eng, cube, seeds, offs, wt, tree[:total], stats[:total])
        # refused calls
        tree.fill_(SENTINEL)
        stats.fill_(SENTINEL64)
        labels = torch.full((s, h, w), SENTINEL, dtype=torch.int32, device=eng.device)
        kw = dict(labels_ptr=labels.data_ptr(), weight_ptr=d_wt.data_ptr(), dtype=U16)
        assert _raw_device(pkg, eng, None, shape, seeds.data_ptr(), offs, tree.data_ptr(), stats.data_ptr(), **kw) == BAD
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, None, offs, tree.data_ptr(), stats.data_ptr(), **kw) == BAD
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs, None, stats.data_ptr(), **kw) == BAD
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs, tree.data_ptr(), None, **kw) == BAD
        assert _raw_device(*args, null_opt=True, **kw) == BAD
        assert _raw_device(*args, row_stride=w - 1, **kw) == BAD
        assert _raw_device(*args, slice_stride=h * w - 1, **kw) == BAD
        assert _raw_device(*args, wrow=w - 1, wslice=h * w, **kw) == BAD                      # a short weight row stride
        assert _raw_device(*args, wslice=h * w - 1, **kw) == BAD                              # a short weight slice stride
        assert _raw_device(*args, wrow=w + 2, wslice=h * (w + 2) - 1, **kw) == BAD
        for bad_dtype in (F.WS_DTYPES["float32"], F.WS_DTYPES["int16"], F.WS_DTYPES["int32"], 17, -1):
            assert _raw_device(*args, labels_ptr=labels.data_ptr(), weight_ptr=d_wt.data_ptr(), dtype=bad_dtype) == F.WS_ERR_UNSUPPORTED
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs[:2] + [offs[1] - 1] + offs[3:], tree.data_ptr(),
                           stats.data_ptr(), **kw) == BAD
        assert _raw_device(*args, opt=eng.options(max_level=255), **kw) == F.WS_ERR_MAX_TOO_HIGH
        assert _raw_device(*args, opt=eng.options(max_level=0), **kw) == F.WS_ERR_MAX_TOO_LOW
        # sizes only: a slice of 0x7FFFFFF0 x 1 pixels passes the plane's bound, its weighted row moment cannot fit 64 bits
        tall = 0x7FFFFFF0
        assert _raw_device(pkg, eng, cube.data_ptr(), (2, tall, 1), seeds.data_ptr(), [0, 1, 2], tree.data_ptr(), stats.data_ptr(),
                           **kw) == F.WS_ERR_TOO_LARGE
        assert _raw_device(pkg, eng, cube.data_ptr(), (2, tall, 1), seeds.data_ptr(), [0, 1, 2], tree.data_ptr(), stats.data_ptr(),
                           labels_ptr=labels.data_ptr()) == F.WS_ERR_TOO_LARGE
        out = torch.empty((h, w), dtype=torch.int32, device=eng.device)
        eng.segment_begin(cube[0], seeds[offs[0]:offs[1]], out)      # a transform in flight is refused
        try:
            assert _raw_device(*args, **kw) == BAD
        finally:
            eng.segment_end()
        torch.cuda.synchronize()
        assert bool((tree == SENTINEL).all()) and bool((stats == SENTINEL64).all()) and bool((labels == SENTINEL).all())
        # no slice: nothing is written
        assert _raw_device(pkg, eng, None, (0, h, w), None, [0], None, None) == 0
        empty = eng.merge_tree_stats_batch(cube[:0], seeds[:0], [0])
        assert tuple(empty[0].shape) == (0, 4) and tuple(empty[1].shape) == (0, 9)


def test_several_groups_equal_one(pkg, torch):
    shape = (7, 128, 96)
    s, h, w = shape
    eng = _engine(pkg)
    imgs = bc.random_images(shape, 4600)
    lists = [np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2) for im in imgs]
    wt = bc.weight_cubes(shape, 48)[2][1]
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    d_wt = _wt_dev(torch, eng, wt)
    one = [t.clone() for t in eng.merge_tree_stats_batch(cube, seeds, offs, weights=d_wt, want_labels=True)]
    one_relax = eng.stats()["launches_relax"]
    eng.ctx.set_batch_pixel_limit(3 * h * w)                        # 3 + 3 + 1 slices
    try:
        groups = eng.merge_tree_stats_batch(cube, seeds, offs, weights=d_wt, want_labels=True)
        groups_relax = eng.stats()["launches_relax"]
    finally:
        eng.ctx.set_batch_pixel_limit(0)
    assert all(torch.equal(a, b) for a, b in zip(groups, one))
    assert groups_relax > one_relax                                 # three floods, not one
    _check_slices_against_single_calls(torch, eng, cube, seeds, offs, wt, *groups)


@pytest.mark.parametrize("shape", [(6, 128, 96), (5, 130, 98)])      # a stack, and the loop
def test_failing_slice_is_named(pkg, torch, shape):
    s, h, w = shape
    eng = _engine(pkg)
    imgs = bc.random_images(shape, 4700)
    wt = bc.weight_cubes(shape, 49)[2][1]
    d_wt = _wt_dev(torch, eng, wt)
    lists = [np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2) for im in imgs]
    lists[3] = np.concatenate([lists[3], np.array([[4000, 3]], np.int64)])
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    total = _first(offs)[-1]
    tree = torch.empty((total, 4), dtype=torch.int32, device=eng.device)
    stats = torch.empty((total, 9), dtype=torch.int64, device=eng.device)
    failed = ctypes.c_size_t(99)
    rc = _raw_device(pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs, tree.data_ptr(), stats.data_ptr(), weight_ptr=d_wt.data_ptr(),
                     dtype=pkg._ffi.WS_DTYPES["uint16"], failed=failed)
    assert rc == pkg._ffi.WS_ERR_SEED_OOB and failed.value == 3, (shape, rc, failed.value)
    # ... and the context works on
    lists[3] = lists[3][:-1]
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    _check_slices_against_single_calls(torch, eng, cube, seeds, offs, wt, *eng.merge_tree_stats_batch(cube, seeds, offs, weights=d_wt))


@pytest.mark.parametrize("shape,edge", [((4, 128, 96), False), ((4, 75, 101), True)])
def test_strided_cubes_and_weight_cubes(pkg, torch, shape, edge):
    """Image and weight cubes both strided and offset, with different strides.  A contiguous image with a strided weight cube still
    stacks (128 x 96); a strided image takes the loop: the records are equal either way."""
    s, h, w = shape
    eng = _engine(pkg)
    F = pkg._ffi
    imgs = bc.random_images(shape, 4800)
    lists = bc.seed_lists(imgs)
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    total = _first(offs)[-1]
    rs, ss = w + 3, h * (w + 3) + 77
    backing, off, _ = strided.embed_cube(np.stack(imgs), 3, rs, ss, 0x00)      # (offset 3: an unaligned base)
    t_back = torch.from_numpy(backing).to(eng.device)
    e = 2 if edge else 0
    for name, wt in bc.weight_cubes(shape, 50)[1:]:
        item = wt.dtype.itemsize
        wrs, wss = w + 5, h * (w + 5) + 31
        woff = 7
        wback = np.random.default_rng(6).integers(0, 256, (woff + s * wss + 16) * item, dtype=np.uint8).view(wt.dtype)
        wview = np.lib.stride_tricks.as_strided(wback[woff:], shape=(s, h, w), strides=(wss * item, wrs * item, item))
        wview[...] = wt
        t_wback = torch.from_numpy(wback.view(np.uint8)).to(eng.device)
        want = [t.clone() for t in eng.merge_tree_stats_batch(cube, seeds, offs, weights=_wt_dev(torch, eng, wt), edge=edge, want_labels=True)]
        want_relax = eng.stats()["launches_relax"]
        _check_slices_against_single_calls(torch, eng, cube, seeds, offs, wt, *want, edge=edge)
        relax = {}
        for strided_image in (False, True):
            tree = torch.full((total + 8, 4), SENTINEL, dtype=torch.int32, device=eng.device)
            stats = torch.full((total + 8, 9), SENTINEL64, dtype=torch.int64, device=eng.device)
            labels = torch.empty((s, h + e, w + e), dtype=torch.int32, device=eng.device)
            rc = _raw_device(pkg, eng, t_back.data_ptr() + off if strided_image else cube.data_ptr(), shape, seeds.data_ptr(), offs,
                             tree.data_ptr(), stats.data_ptr(), labels.data_ptr(), weight_ptr=t_wback.data_ptr() + woff * item,
                             dtype=F.WS_DTYPES[wt.dtype.name], wrow=wrs, wslice=wss, edge=edge,
                             row_stride=rs if strided_image else None, slice_stride=ss if strided_image else None)
            assert rc == 0
            relax[strided_image] = eng.stats()["launches_relax"]
            assert torch.equal(tree[:total], want[0]) and bool((tree[total:] == SENTINEL).all()), (name, strided_image)
            assert torch.equal(stats[:total], want[1]) and bool((stats[total:] == SENTINEL64).all()), (name, strided_image)
            assert torch.equal(labels, want[2])
        if shape == (4, 128, 96):      # strided weights still stack (one flood), a strided image takes the loop (four)
            assert relax[False] < relax[True] and want_relax < relax[True], (relax, want_relax)
    # no weight cube: the strided image cube itself weighs
    want = [t.clone() for t in eng.merge_tree_stats_batch(cube, seeds, offs, edge=edge)]
    tree = torch.empty((total, 4), dtype=torch.int32, device=eng.device)
    stats = torch.empty((total, 9), dtype=torch.int64, device=eng.device)
    assert _raw_device(pkg, eng, t_back.data_ptr() + off, shape, seeds.data_ptr(), offs, tree.data_ptr(), stats.data_ptr(), dtype=99, edge=edge,
                       row_stride=rs, slice_stride=ss) == 0
    assert torch.equal(tree, want[0]) and torch.equal(stats, want[1])
    host = _ws(pkg, edge=edge).merge_tree_stats_cube(strided.view_cube(backing, off, s, h, w, rs, ss), seeds=[l.astype(np.uint64) for l in lists])
    assert ls.mismatch(np.concatenate([r for _, r in host]), _rec(want[1])) is None


def test_alternating_calls_on_one_context(pkg, torch):
    """stats batch, tree batch, history batch, single stats, stats batch again: the stacked statistics call uses the stacked
    history loop's graphs, and none of the others is changed by the interleaving."""
    eng = _engine(pkg)
    shape = (4, 128, 96)
    imgs = bc.random_images(shape, 4900)
    lists = [np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2) for im in imgs]
    wt = bc.weight_cubes(shape, 51)[2][1]
    d_wt = _wt_dev(torch, eng, wt)
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    levels = [254, 0, 77, 160]

    def stats_batch():
        return [t.clone() for t in eng.merge_tree_stats_batch(cube, seeds, offs, weights=d_wt)]

    def tree_batch():
        return [eng.merge_tree_batch(cube, seeds, offs).clone()]

    def history_batch():
        return [eng.transform_history_batch(cube, seeds, offs, levels=levels, merging=True).clone()]

    def single_stats():
        return [t.clone() for t in eng.merge_tree_stats(cube[2], seeds[offs[2]:offs[3]], weights=d_wt[2])]

    first = {}
    for rep in range(3):
        for fn in (stats_batch, tree_batch, history_batch, single_stats, stats_batch):
            got = fn()
            torch.cuda.synchronize()
            want = first.setdefault(fn.__name__, got)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (rep, fn.__name__)
    # three stats batches in a row: captured by the second, replayed by the third -- every group of 16 levels a graph launch
    for _ in range(3):
        got = stats_batch()
        assert all(torch.equal(a, b) for a, b in zip(got, first["stats_batch"]))
    assert eng.stats()["graph_launches"] >= 16, eng.stats()["graph_launches"]
    assert torch.equal(first["stats_batch"][0], first["tree_batch"][0])
    f = _first(offs)
    assert torch.equal(first["stats_batch"][1][f[2]:f[3]], first["single_stats"][1])
    _check_slices_against_single_calls(torch, eng, cube, seeds, offs, wt, *first["stats_batch"])


def _rows(t):
    return np.stack([t.parent, t.death_level, t.area, t.n_leaves], axis=1)


@pytest.mark.parametrize("shape", [(5, 128, 112), (5, 130, 98)])      # a stack, and the loop
def test_host_form_equals_device_form_and_slice_calls(pkg, torch, shape):
    s, h, w = shape
    eng = _engine(pkg)
    imgs = bc.random_images(shape, 5000)
    cube = np.stack(imgs)
    ws = _ws(pkg, max_level=200)
    for name, wt in bc.weight_cubes(shape, 52):
        got, counts = ws.merge_tree_stats_cube(cube, weights=wt, want_labels=True)      # every slice's own minima
        mins = [ws.find_local_minima(cube[k]) for k in range(s)]
        lists = list(mins)
        lists[1] = lists[1][:0]
        lists[2] = lists[2][:1]
        given = ws.merge_tree_stats_cube(cube, seeds=lists, weights=wt)
        assert len(got) == len(given) == s
        d_cube, d_seeds, offs = _device_inputs(torch, eng, imgs, [np.asarray(l, dtype=np.int64).reshape(-1, 2) for l in lists])
        d_tree, d_stats = eng.merge_tree_stats_batch(d_cube, d_seeds, offs, weights=_wt_dev(torch, eng, wt), max_level=200)
        torch.cuda.synchronize()
        assert (np.concatenate([_rows(t) for t, _ in given]) == _u32(d_tree)).all(), name
        assert ls.mismatch(np.concatenate([r for _, r in given]), _rec(d_stats)) is None, name
        for k in range(s):
            assert counts[k] == len(mins[k])
            assert got[k][1].dtype == pkg.api.LAKE_STATS_DTYPE
            want_tree, want = ws.merge_tree_stats(cube[k], mins[k], weights=None if wt is None else wt[k], want_labels=True)
            assert (_rows(got[k][0]) == _rows(want_tree)).all() and ls.mismatch(got[k][1], want) is None, (name, k)
            assert got[k][0].labels.dtype == np.uint64 and (got[k][0].labels == want_tree.labels).all(), k
            want_tree, want = ws.merge_tree_stats(cube[k], lists[k], weights=None if wt is None else wt[k])
            assert given[k][0].labels is None and (_rows(given[k][0]) == _rows(want_tree)).all() and ls.mismatch(given[k][1], want) is None, (name, k)
    # the raw call with room for one record less: the count, and nothing else
    L = pkg._ffi.lib()
    total = int(sum(counts)) + s
    tree = np.full((total, 4), SENTINEL, dtype=np.uint32)
    stats = np.full(total * 9, SENTINEL64, dtype=np.uint64)
    labels = np.full((s, h, w), SENTINEL, dtype=np.uint64)
    n_rec, failed = ctypes.c_size_t(0), ctypes.c_size_t(0)
    n_seeds = np.zeros(s, dtype=np.uintp)
    ctx = ws._ctx()
    wt = np.ascontiguousarray(bc.weight_cubes(shape, 52)[2][1])
    args = (ctx.handle, cube.ctypes.data, s, h, w, w, h * w, None, None, ctypes.byref(ws._opt), wt.ctypes.data, pkg._ffi.WS_DTYPES["uint16"], w,
            h * w, tree.ctypes.data, stats.ctypes.data)
    tail = (ctypes.byref(n_rec), labels.ctypes.data, n_seeds.ctypes.data_as(pkg._ffi.szp), ctypes.byref(failed))
    assert L.ws_merge_tree_stats_batch(*args, total - 1, *tail) == pkg._ffi.WS_ERR_CAPACITY
    assert n_rec.value == total and (n_seeds == counts).all()
    assert (tree == SENTINEL).all() and (stats == SENTINEL64).all() and (labels == SENTINEL).all()
    assert L.ws_merge_tree_stats_batch(*args, total, *tail) == 0
    assert n_rec.value == total and (tree == np.concatenate([_rows(t) for t, _ in got])).all()
    assert ls.mismatch(stats.view(ls.DTYPE), np.concatenate([r for _, r in got])) is None
    assert (labels == np.stack([t.labels for t, _ in got])).all()


def test_torch_mirror_reuses_out_and_refuses_wrong_shapes(pkg, torch):
    eng = _engine(pkg)
    shape = (4, 126, 94)
    imgs = [cases.smooth_field(shape[1], shape[2], 5100 + k) for k in range(shape[0])]
    lists = [np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2) for im in imgs]
    wt = bc.weight_cubes(shape, 53)[1][1]
    d_wt = _wt_dev(torch, eng, wt)
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    total = _first(offs)[-1]
    out = torch.full((total, 4), -7, dtype=torch.int32, device=eng.device)
    out_stats = torch.full((total, 9), -7, dtype=torch.int64, device=eng.device)
    tree, stats, labels = eng.merge_tree_stats_batch(cube, seeds, offs, weights=d_wt, edge=True, want_labels=True, out=out, out_stats=out_stats)
    assert tree.data_ptr() == out.data_ptr() and stats.data_ptr() == out_stats.data_ptr()
    assert tuple(stats.shape) == (total, 9) and stats.dtype == torch.int64 and tuple(labels.shape) == (4, 128, 96)
    _check_slices_against_single_calls(torch, eng, cube, seeds, offs, wt, tree, stats, labels, edge=True)
    again = eng.merge_tree_stats_batch(cube, seeds, offs, weights=d_wt, edge=True, out=out, out_stats=out_stats)
    assert again[0].data_ptr() == out.data_ptr() and again[1].data_ptr() == out_stats.data_ptr()
    host = _ws(pkg, edge=True).merge_tree_stats_cube(np.stack(imgs), seeds=[l.astype(np.uint64) for l in lists], weights=wt)
    assert ls.mismatch(np.concatenate([r for _, r in host]), _rec(stats)) is None
    with pytest.raises(ValueError):
        eng.merge_tree_stats_batch(cube, seeds, offs, out=torch.empty((total + 1, 4), dtype=torch.int32, device=eng.device))
    with pytest.raises(ValueError):
        eng.merge_tree_stats_batch(cube, seeds, offs, out_stats=torch.empty((total, 8), dtype=torch.int64, device=eng.device))
    with pytest.raises(ValueError):
        eng.merge_tree_stats_batch(cube, seeds, offs, weights=d_wt[:, :, :90])
    with pytest.raises(TypeError):
        eng.merge_tree_stats_batch(cube, seeds, offs, weights=d_wt.to(torch.float32))


def test_stack_is_taken_at_size(pkg, torch):
    s, h, w = 16, 1024, 1024
    eng = _engine(pkg)
    cube = torch.stack([eng.random_field(h, w, 5200 + k) for k in range(s)]).contiguous()
    lists = [eng.find_local_minima(cube[k]) for k in range(s)]
    offs = [0] + [int(x) for x in np.cumsum([int(l.shape[0]) for l in lists])]
    seeds = torch.cat(lists).contiguous()
    g = torch.Generator(device="cpu").manual_seed(52)
    d_wt = torch.randint(-32768, 32768, (s, h, w), generator=g, dtype=torch.int16).to(eng.device)      # u16 bits
    tree, stats = eng.merge_tree_stats_batch(cube, seeds, offs, weights=d_wt)
    batch_relax = eng.stats()["launches_relax"]
    first = _first(offs)
    loop_relax = 0
    totals = (d_wt.to(torch.int64) & 0xFFFF).sum(dim=(1, 2))
    for k in range(s):
        one_tree, one_stats = eng.merge_tree_stats(cube[k], lists[k], weights=d_wt[k])
        loop_relax += eng.stats()["launches_relax"]
        t, r = tree[first[k]:first[k + 1]], stats[first[k]:first[k + 1]]
        assert torch.equal(t, one_tree) and torch.equal(r, one_stats), k
        alive = (t[:, 1] == -1) & (t[:, 3] > 0)
        alive[0] = True
        assert int(r[alive, 0].sum()) == int(totals[k]), k      # the survivors' sum_w and record 0's: the slice's total weight
    assert batch_relax < loop_relax, (batch_relax, loop_relax)      # one stacked flood, not sixteen
