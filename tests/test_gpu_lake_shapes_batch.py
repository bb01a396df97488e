"""merge_tree_shapes of a cube of slices in one call (ws_merge_tree_shapes_batch(_device)), -m gpu.  The yardsticks are never the
batch itself: all twelve words of every record against the Python-integer reference of tests/lake_shapes_ref.py over the CPU
oracle's planes (or a closed form), the tree and the statistics byte for byte against ws_merge_tree_stats_batch_device, every slice
against ws_merge_tree_shapes_device on that slice alone with that slice's weight plane.  tests/test_lake_shapes_batch_cpu.py proves
what the cubes of tests/lake_shapes_batch_cases.py are there for.  Every comparison is on integers and bit for bit."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import lake_shapes_batch_cases as sbc
import lake_shapes_ref as sh
import lake_stats_batch_cases as bc
import oracle_lib as ol
import strided

pytestmark = pytest.mark.gpu

PAT32 = 0x5A5A5A5A
PAT = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def eng(pkg, torch):
    with torch.cuda.stream(torch.cuda.Stream(0)):      # a stream of its own: the level loops are captured and replayed
        yield importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


def _ws(pkg, max_level=254, edge=False, seed_shift=False):
    b = pkg.TransformBuilder.new().set_max_water_lvl(max_level)
    if edge:
        b.enable_edge_correction()
    if seed_shift:
        b.shift_seeds_into_padded_plane()
    return b.build_merging()


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return _np(a).tobytes() == _np(b).tobytes()


def _wt_dev(torch, eng, wt):
    """A u8 cube (or plane) as it is, a u16 one as its int16 bits; None stays None."""
    if wt is None:
        return None
    wt = np.ascontiguousarray(wt)
    return torch.from_numpy(wt if wt.dtype == np.uint8 else wt.view(np.int16)).to(eng.device)


def _inputs(torch, eng, imgs, lists):
    lists = [np.asarray(l, dtype=np.int64).reshape(-1, 2) for l in lists]
    flat = np.concatenate(lists, axis=0) if sum(len(l) for l in lists) else np.zeros((0, 2), np.int64)
    offs = [0] + [int(x) for x in np.cumsum([len(l) for l in lists])]
    cube = torch.from_numpy(np.stack(imgs)).to(eng.device).contiguous()
    return cube, torch.from_numpy(flat.astype(np.int32)).to(eng.device).contiguous(), offs


def _first(offs):
    return [int(offs[k]) - int(offs[0]) + k for k in range(len(offs))]


def _kw(c):
    return dict(max_level=c.max_level, edge=c.edge, seed_shift=c.seed_shift)


def _check_against_stats_batch_and_single_calls(torch, eng, cube, seeds, offs, wt, got, labels=None, **kw):
    """tree and stats of the shapes call byte for byte against the stats batch call; every slice's three record arrays (and
    labels) against merge_tree_shapes on that slice alone with its own weight plane."""
    d_wt = _wt_dev(torch, eng, wt)
    tree, stats, shapes = got
    want = eng.merge_tree_stats_batch(cube, seeds, offs, weights=d_wt, want_labels=True, **kw)
    torch.cuda.synchronize()
    assert _same(tree, want[0]) and _same(stats, want[1]), "tree and stats against the stats batch call"
    if labels is not None:
        assert _same(labels, want[2])
    first = _first(offs)
    assert tuple(shapes.shape) == (first[-1], 12) and shapes.dtype == torch.int64
    for k in range(cube.shape[0]):
        one = eng.merge_tree_shapes(cube[k], seeds[offs[k]:offs[k + 1]], weights=None if d_wt is None else d_wt[k], want_labels=True, **kw)
        torch.cuda.synchronize()
        rows = slice(first[k], first[k + 1])
        assert _same(tree[rows], one[0]) and _same(stats[rows], one[1]), k
        assert _same(shapes[rows], one[2]), (k, sh.mismatch(_np(shapes[rows]), sh.from_words(_np(one[2]))))
        if labels is not None:
            assert _same(labels[k], one[3]), k


def _run_case(torch, eng, name):
    c = sbc.cube(name)
    cube, seeds, offs = _inputs(torch, eng, c.imgs, c.lists)
    tree, stats, shapes, labels = eng.merge_tree_shapes_batch(cube, seeds, offs, weights=_wt_dev(torch, eng, c.weights), want_labels=True, **_kw(c))
    torch.cuda.synchronize()
    return c, cube, seeds, offs, tree, stats, shapes, labels


@pytest.mark.parametrize("name", sbc.ORACLE_CASES)
def test_every_record_against_the_reference_the_stats_batch_and_single_calls(torch, eng, name):
    c, cube, seeds, offs, tree, stats, shapes, labels = _run_case(torch, eng, name)
    want = sbc.expected_sums(name)
    assert sh.mismatch(_np(shapes), want) is None, (name, sh.mismatch(_np(shapes), want))
    refs = sbc.reference(name)
    assert (_np(tree).view(np.uint32) == np.concatenate([r.tree for r in refs])).all(), name
    assert c.first() == _first(offs)
    _check_against_stats_batch_and_single_calls(torch, eng, cube, seeds, offs, c.weights, (tree, stats, shapes), labels, **_kw(c))
    if name.startswith("shape:"):      # the seedless slice owns its record 0 alone
        f = c.first()
        assert f[2] - f[1] == 1 and f[3] - f[2] == 2


def test_high_word_and_the_stacked_instantiation_that_is_not_flat(torch, eng):
    """Two slices of 8 x 70016 (tests/test_lake_shapes_batch_cpu.py: they stack, a side passes 65 535, the sum of v col^2 of each
    slice's lake passes 2^64): closed forms, no oracle run."""
    c, cube, seeds, offs, tree, stats, shapes, labels = _run_case(torch, eng, "high_word")
    want = sbc.expected_sums("high_word")
    assert sh.mismatch(_np(shapes), want) is None, sh.mismatch(_np(shapes), want)
    got = sh.from_words(_np(shapes))
    assert got[1][1] >= 1 << 64 and got[3][1] >= 1 << 64
    assert (_np(tree).view(np.uint32) == np.concatenate([sbc.high_word_expected(k)[0] for k in range(2)])).all()
    _check_against_stats_batch_and_single_calls(torch, eng, cube, seeds, offs, c.weights, (tree, stats, shapes), labels, **_kw(c))


def _raw_device(pkg, eng, cube_ptr, shape, seeds_ptr, offs, tree_ptr, stats_ptr, shapes_ptr, labels_ptr=None, weight_ptr=None, dtype=0, wrow=None,
                wslice=None, max_level=254, edge=False, failed=None, row_stride=None, slice_stride=None, opt=None, null_opt=False):
    """ws_merge_tree_shapes_batch_device itself."""
    import torch
    s, h, w = shape
    opt = opt if opt is not None else eng.options(max_level, edge)
    c_offs = (ctypes.c_size_t * (len(offs)))(*[int(x) for x in offs])
    rs = w if row_stride is None else row_stride
    wr = w if wrow is None else wrow
    rc = pkg._ffi.lib().ws_merge_tree_shapes_batch_device(eng.ctx.handle, cube_ptr, s, h, w, rs, h * rs if slice_stride is None else slice_stride,
                                                          seeds_ptr, c_offs, None if null_opt else ctypes.byref(opt), weight_ptr, dtype, wr,
                                                          h * wr if wslice is None else wslice, tree_ptr, stats_ptr, shapes_ptr, labels_ptr,
                                                          ctypes.byref(failed) if failed is not None else None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("shape,edge", [((4, 128, 96), False), ((4, 75, 101), True)])
def test_strided_cubes_and_weight_cubes(pkg, torch, eng, shape, edge):
    """u8 and u16 weight cubes with odd row and slice strides of their own, and no weights.  A contiguous image with a strided
    weight cube still stacks (128 x 96); a cube view with slice_stride != h * row_stride takes the loop: the same records."""
    s, h, w = shape
    F = pkg._ffi
    imgs = bc.random_images(shape, 4800)
    lists = bc.seed_lists(imgs)
    cube, seeds, offs = _inputs(torch, eng, imgs, lists)
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
        want = [t.clone() for t in eng.merge_tree_shapes_batch(cube, seeds, offs, weights=_wt_dev(torch, eng, wt), edge=edge, want_labels=True)]
        want_relax = eng.stats()["launches_relax"]
        _check_against_stats_batch_and_single_calls(torch, eng, cube, seeds, offs, wt, want[:3], want[3], edge=edge)
        relax = {}
        for strided_image in (False, True):
            tree = torch.full((total + 8, 4), PAT32, dtype=torch.int32, device=eng.device)
            stats = torch.full((total + 8, 9), PAT, dtype=torch.int64, device=eng.device)
            shapes = torch.full((total + 8, 12), PAT, dtype=torch.int64, device=eng.device)
            labels = torch.empty((s, h + e, w + e), dtype=torch.int32, device=eng.device)
            rc = _raw_device(pkg, eng, t_back.data_ptr() + off if strided_image else cube.data_ptr(), shape, seeds.data_ptr(), offs,
                             tree.data_ptr(), stats.data_ptr(), shapes.data_ptr(), labels.data_ptr(), weight_ptr=t_wback.data_ptr() + woff * item,
                             dtype=F.WS_DTYPES[wt.dtype.name], wrow=wrs, wslice=wss, edge=edge,
                             row_stride=rs if strided_image else None, slice_stride=ss if strided_image else None)
            assert rc == 0
            relax[strided_image] = eng.stats()["launches_relax"]
            assert torch.equal(tree[:total], want[0]) and bool((tree[total:] == PAT32).all()), (name, strided_image)
            assert torch.equal(stats[:total], want[1]) and bool((stats[total:] == PAT).all()), (name, strided_image)
            assert torch.equal(shapes[:total], want[2]) and bool((shapes[total:] == PAT).all()), (name, strided_image)
            assert torch.equal(labels, want[3])
        if shape == (4, 128, 96):      # strided weights still stack (one flood), a strided image takes the loop (four)
            assert relax[False] < relax[True] and want_relax < relax[True], (relax, want_relax)
    # no weight cube: the strided image cube itself weighs
    want = [t.clone() for t in eng.merge_tree_shapes_batch(cube, seeds, offs, edge=edge)]
    _check_against_stats_batch_and_single_calls(torch, eng, cube, seeds, offs, None, want, edge=edge)
    tree = torch.empty((total, 4), dtype=torch.int32, device=eng.device)
    stats = torch.empty((total, 9), dtype=torch.int64, device=eng.device)
    shapes = torch.empty((total, 12), dtype=torch.int64, device=eng.device)
    assert _raw_device(pkg, eng, t_back.data_ptr() + off, shape, seeds.data_ptr(), offs, tree.data_ptr(), stats.data_ptr(), shapes.data_ptr(), dtype=99,
                       edge=edge, row_stride=rs, slice_stride=ss) == 0
    assert torch.equal(tree, want[0]) and torch.equal(stats, want[1]) and torch.equal(shapes, want[2])


def test_several_groups_equal_one(torch, eng):
    shape = (7, 128, 96)
    s, h, w = shape
    imgs = bc.random_images(shape, 4600)
    lists = [np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2) for im in imgs]
    wt = bc.weight_cubes(shape, 48)[2][1]
    cube, seeds, offs = _inputs(torch, eng, imgs, lists)
    d_wt = _wt_dev(torch, eng, wt)
    one = [t.clone() for t in eng.merge_tree_shapes_batch(cube, seeds, offs, weights=d_wt, want_labels=True)]
    one_relax = eng.stats()["launches_relax"]
    eng.ctx.set_batch_pixel_limit(3 * h * w)                        # 3 + 3 + 1 slices
    try:
        groups = eng.merge_tree_shapes_batch(cube, seeds, offs, weights=d_wt, want_labels=True)
        groups_relax = eng.stats()["launches_relax"]
    finally:
        eng.ctx.set_batch_pixel_limit(0)
    assert all(torch.equal(a, b) for a, b in zip(groups, one))
    assert groups_relax > one_relax                                 # three floods, not one
    _check_against_stats_batch_and_single_calls(torch, eng, cube, seeds, offs, wt, groups[:3], groups[3])


@pytest.mark.parametrize("shape", [(6, 128, 96), (5, 130, 98)])      # a stack, and the loop
def test_failing_slice_is_named(pkg, torch, eng, shape):
    imgs = bc.random_images(shape, 4700)
    wt = bc.weight_cubes(shape, 49)[2][1]
    d_wt = _wt_dev(torch, eng, wt)
    lists = [np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2) for im in imgs]
    lists[3] = np.concatenate([lists[3], np.array([[4000, 3]], np.int64)])
    cube, seeds, offs = _inputs(torch, eng, imgs, lists)
    total = _first(offs)[-1]
    tree = torch.empty((total, 4), dtype=torch.int32, device=eng.device)
    stats = torch.empty((total, 9), dtype=torch.int64, device=eng.device)
    shapes = torch.empty((total, 12), dtype=torch.int64, device=eng.device)
    failed = ctypes.c_size_t(99)
    rc = _raw_device(pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs, tree.data_ptr(), stats.data_ptr(), shapes.data_ptr(),
                     weight_ptr=d_wt.data_ptr(), dtype=pkg._ffi.WS_DTYPES["uint16"], failed=failed)
    assert rc == pkg._ffi.WS_ERR_SEED_OOB and failed.value == 3, (shape, rc, failed.value)
    # ... and the context works on
    lists[3] = lists[3][:-1]
    cube, seeds, offs = _inputs(torch, eng, imgs, lists)
    _check_against_stats_batch_and_single_calls(torch, eng, cube, seeds, offs, wt, eng.merge_tree_shapes_batch(cube, seeds, offs, weights=d_wt))


def test_only_the_calls_records_are_written_and_refusals_touch_nothing(pkg, torch, eng):
    F = pkg._ffi
    BAD = F.WS_ERR_BAD_ARG
    U16 = F.WS_DTYPES["uint16"]
    for shape in ((4, 128, 96), (4, 130, 98)):
        s, h, w = shape
        imgs = bc.random_images(shape, 4500)
        lists = bc.seed_lists(imgs)
        wt = bc.weight_cubes(shape, 47)[2][1]
        cube, seeds, offs = _inputs(torch, eng, imgs, lists)
        d_wt = _wt_dev(torch, eng, wt)
        total = _first(offs)[-1]
        # the records in the middle of pre-filled arrays: pattern words stay before and after them
        tree = torch.full((total + 64, 4), PAT32, dtype=torch.int32, device=eng.device)
        stats = torch.full((total + 64, 9), PAT, dtype=torch.int64, device=eng.device)
        shapes = torch.full((total + 64, 12), PAT, dtype=torch.int64, device=eng.device)
        lead = 32
        mid = slice(lead, lead + total)
        ptrs = (tree[lead:].data_ptr(), stats[lead:].data_ptr(), shapes[lead:].data_ptr())
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs, *ptrs, weight_ptr=d_wt.data_ptr(), dtype=U16) == 0
        for t, pat in ((tree, PAT32), (stats, PAT), (shapes, PAT)):
            assert bool((t[:lead] == pat).all()) and bool((t[lead + total:] == pat).all())
        _check_against_stats_batch_and_single_calls(torch, eng, cube, seeds, offs, wt, (tree[mid], stats[mid], shapes[mid]))
        # offsets that do not start at 0: the records still start at the front of the arrays
        for t, pat in ((tree, PAT32), (stats, PAT), (shapes, PAT)):
            t.fill_(pat)
        shifted = [o + 5 for o in offs]
        pad = torch.cat([torch.zeros((5, 2), dtype=torch.int32, device=eng.device), seeds]).contiguous()
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, pad.data_ptr(), shifted, tree.data_ptr(), stats.data_ptr(), shapes.data_ptr(),
                           weight_ptr=d_wt.data_ptr(), dtype=U16) == 0
        assert bool((tree[total:] == PAT32).all()) and bool((stats[total:] == PAT).all()) and bool((shapes[total:] == PAT).all())
        _check_against_stats_batch_and_single_calls(torch, eng, cube, seeds, offs, wt, (tree[:total], stats[:total], shapes[:total]))
        # refused calls
        for t, pat in ((tree, PAT32), (stats, PAT), (shapes, PAT)):
            t.fill_(pat)
        labels = torch.full((s, h, w), PAT32, dtype=torch.int32, device=eng.device)
        kw = dict(labels_ptr=labels.data_ptr(), weight_ptr=d_wt.data_ptr(), dtype=U16)
        args = (pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs, tree.data_ptr(), stats.data_ptr(), shapes.data_ptr())
        p = (tree.data_ptr(), stats.data_ptr(), shapes.data_ptr())
        assert _raw_device(pkg, eng, None, shape, seeds.data_ptr(), offs, *p, **kw) == BAD
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, None, offs, *p, **kw) == BAD
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs, None, p[1], p[2], **kw) == BAD
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs, p[0], None, p[2], **kw) == BAD
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs, p[0], p[1], None, **kw) == BAD          # a null d_shapes
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs, p[0], p[1], p[2] + 4, **kw) == BAD      # off 8-byte alignment
        assert _raw_device(*args, null_opt=True, **kw) == BAD
        assert _raw_device(*args, row_stride=w - 1, **kw) == BAD
        assert _raw_device(*args, slice_stride=h * w - 1, **kw) == BAD
        assert _raw_device(*args, wrow=w - 1, wslice=h * w, **kw) == BAD                      # a short weight row stride
        assert _raw_device(*args, wslice=h * w - 1, **kw) == BAD                              # a short weight slice stride
        for bad_dtype in (F.WS_DTYPES["float32"], F.WS_DTYPES["int16"], 17, -1):
            assert _raw_device(*args, labels_ptr=labels.data_ptr(), weight_ptr=d_wt.data_ptr(), dtype=bad_dtype) == F.WS_ERR_UNSUPPORTED
        assert _raw_device(pkg, eng, cube.data_ptr(), shape, seeds.data_ptr(), offs[:2] + [offs[1] - 1] + offs[3:], *p, **kw) == BAD
        assert _raw_device(*args, opt=eng.options(max_level=255), **kw) == F.WS_ERR_MAX_TOO_HIGH
        assert _raw_device(*args, opt=eng.options(max_level=0), **kw) == F.WS_ERR_MAX_TOO_LOW
        # the stats call's order holds: a plane it refuses as too large is refused so, before the shapes pointer is looked at
        tall = 0x7FFFFFF0
        assert _raw_device(pkg, eng, cube.data_ptr(), (2, tall, 1), seeds.data_ptr(), [0, 1, 2], *p, **kw) == F.WS_ERR_TOO_LARGE
        assert _raw_device(pkg, eng, cube.data_ptr(), (2, tall, 1), seeds.data_ptr(), [0, 1, 2], p[0], p[1], None, **kw) == F.WS_ERR_TOO_LARGE
        out = torch.empty((h, w), dtype=torch.int32, device=eng.device)
        eng.segment_begin(cube[0], seeds[offs[0]:offs[1]], out)      # a transform in flight is refused
        try:
            assert _raw_device(*args, **kw) == BAD
        finally:
            eng.segment_end()
        torch.cuda.synchronize()
        assert bool((tree == PAT32).all()) and bool((stats == PAT).all()) and bool((shapes == PAT).all()) and bool((labels == PAT32).all())
        # no slice: nothing is written
        assert _raw_device(pkg, eng, None, (0, h, w), None, [0], None, None, None) == 0
        assert _raw_device(pkg, eng, cube.data_ptr(), (0, h, w), seeds.data_ptr(), [0], *p, **kw) == 0
        assert bool((tree == PAT32).all()) and bool((stats == PAT).all()) and bool((shapes == PAT).all()) and bool((labels == PAT32).all())
        empty = eng.merge_tree_shapes_batch(cube[:0], seeds[:0], [0])
        assert tuple(empty[0].shape) == (0, 4) and tuple(empty[1].shape) == (0, 9) and tuple(empty[2].shape) == (0, 12)


def test_alternating_calls_on_one_context(torch, eng):
    """shapes batch, stats batch, single shapes, history batch, shapes batch again: none is changed by the interleaving."""
    shape = (4, 128, 96)
    imgs = bc.random_images(shape, 4900)
    lists = [np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2) for im in imgs]
    wt = bc.weight_cubes(shape, 51)[2][1]
    d_wt = _wt_dev(torch, eng, wt)
    cube, seeds, offs = _inputs(torch, eng, imgs, lists)
    levels = [254, 0, 77, 160]

    def shapes_batch():
        return [t.clone() for t in eng.merge_tree_shapes_batch(cube, seeds, offs, weights=d_wt)]

    def stats_batch():
        return [t.clone() for t in eng.merge_tree_stats_batch(cube, seeds, offs, weights=d_wt)]

    def single_shapes():
        return [t.clone() for t in eng.merge_tree_shapes(cube[2], seeds[offs[2]:offs[3]], weights=d_wt[2])]

    def history_batch():
        return [eng.transform_history_batch(cube, seeds, offs, levels=levels, merging=True).clone()]

    seen = {}
    for rep in range(2):
        for fn in (shapes_batch, stats_batch, single_shapes, history_batch, shapes_batch):
            got = fn()
            torch.cuda.synchronize()
            want = seen.setdefault(fn.__name__, got)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (rep, fn.__name__)
    assert all(torch.equal(a, b) for a, b in zip(seen["shapes_batch"][:2], seen["stats_batch"]))
    f = _first(offs)
    assert torch.equal(seen["shapes_batch"][2][f[2]:f[3]], seen["single_shapes"][2])
    _check_against_stats_batch_and_single_calls(torch, eng, cube, seeds, offs, wt, seen["shapes_batch"])


def _rows(t):
    return np.stack([t.parent, t.death_level, t.area, t.n_leaves], axis=1)


@pytest.mark.parametrize("shape", [(5, 128, 112), (5, 130, 98)])      # a stack, and the loop
def test_host_form_cube_api_and_ellipses(pkg, torch, eng, shape):
    s, h, w = shape
    imgs = bc.random_images(shape, 5000)
    cube = np.stack(imgs)
    ws = _ws(pkg, max_level=200)
    for name, wt in bc.weight_cubes(shape, 52):
        got, counts = ws.merge_tree_shapes_cube(cube, weights=wt, want_labels=True)      # every slice's own minima
        mins = [ws.find_local_minima(cube[k]) for k in range(s)]
        assert [int(x) for x in counts] == [len(m) for m in mins]
        explicit = ws.merge_tree_shapes_cube(cube, seeds=mins, weights=wt)              # seeds=None equals explicit minima
        lists = list(mins)
        lists[1] = lists[1][:0]
        lists[2] = lists[2][:1]
        given = ws.merge_tree_shapes_cube(cube, seeds=lists, weights=wt)
        assert len(got) == len(given) == len(explicit) == s
        d_cube, d_seeds, offs = _inputs(torch, eng, imgs, lists)
        d_tree, d_stats, d_shapes = eng.merge_tree_shapes_batch(d_cube, d_seeds, offs, weights=_wt_dev(torch, eng, wt), max_level=200)
        torch.cuda.synchronize()
        assert (np.concatenate([_rows(t) for t, _, _ in given]) == _np(d_tree).view(np.uint32)).all(), name
        assert np.concatenate([r for _, r, _ in given]).tobytes() == _np(d_stats).tobytes(), name
        assert np.concatenate([x for _, _, x in given]).tobytes() == _np(d_shapes).tobytes(), name
        for k in range(s):
            assert got[k][2].dtype == pkg.api.LAKE_SHAPE_DTYPE and got[k][2].shape == (len(mins[k]) + 1,)
            want = ws.merge_tree_shapes(cube[k], mins[k], weights=None if wt is None else wt[k], want_labels=True)
            for res in (got[k], explicit[k]):
                assert (_rows(res[0]) == _rows(want[0])).all() and res[1].tobytes() == want[1].tobytes() and res[2].tobytes() == want[2].tobytes(), (name, k)
            assert got[k][0].labels.dtype == np.uint64 and (got[k][0].labels == want[0].labels).all() and explicit[k][0].labels is None
            want = ws.merge_tree_shapes(cube[k], lists[k], weights=None if wt is None else wt[k])
            assert given[k][1].tobytes() == want[1].tobytes() and given[k][2].tobytes() == want[2].tobytes(), (name, k)
        # ellipses on one slice's records, unchanged: equal to ellipses on the single call's
        k = 3
        want = ws.merge_tree_shapes(cube[k], mins[k], weights=None if wt is None else wt[k])
        for a, b in zip(pkg.ellipses(got[k][1], got[k][2]), pkg.ellipses(want[1], want[2])):
            assert np.array_equal(a, b, equal_nan=True)
        for a, b in zip(pkg.ellipses(got[k][1], got[k][2], weighted=False, area=got[k][0].area), pkg.ellipses(want[1], want[2], weighted=False, area=want[0].area)):
            assert np.array_equal(a, b, equal_nan=True)
    # the raw call with room for one record less: the count, and nothing else
    L = pkg._ffi.lib()
    total = int(sum(counts)) + s
    tree = np.full((total, 4), PAT32, dtype=np.uint32)
    stats = np.full(total * 9, PAT, dtype=np.uint64)
    shapes = np.full(total * 12, PAT, dtype=np.uint64)
    labels = np.full((s, h, w), PAT32, dtype=np.uint64)
    n_rec, failed = ctypes.c_size_t(0), ctypes.c_size_t(0)
    n_seeds = np.zeros(s, dtype=np.uintp)
    ctx = ws._ctx()
    wt = np.ascontiguousarray(bc.weight_cubes(shape, 52)[2][1])
    args = (ctx.handle, cube.ctypes.data, s, h, w, w, h * w, None, None, ctypes.byref(ws._opt), wt.ctypes.data, pkg._ffi.WS_DTYPES["uint16"], w,
            h * w, tree.ctypes.data, stats.ctypes.data)
    tail = (ctypes.byref(n_rec), labels.ctypes.data, n_seeds.ctypes.data_as(pkg._ffi.szp), ctypes.byref(failed))
    assert L.ws_merge_tree_shapes_batch(*args, shapes.ctypes.data, total - 1, *tail) == pkg._ffi.WS_ERR_CAPACITY
    assert n_rec.value == total and (n_seeds == counts).all()
    assert (tree == PAT32).all() and (stats == PAT).all() and (shapes == PAT).all() and (labels == PAT32).all()
    assert L.ws_merge_tree_shapes_batch(*args, None, total, *tail) == pkg._ffi.WS_ERR_BAD_ARG          # a null `shapes` with cap != 0
    assert (tree == PAT32).all() and (stats == PAT).all() and (labels == PAT32).all()
    assert L.ws_merge_tree_shapes_batch(*args, shapes.ctypes.data, total, *tail) == 0
    assert n_rec.value == total and (tree == np.concatenate([_rows(t) for t, _, _ in got])).all()
    assert stats.tobytes() == np.concatenate([r for _, r, _ in got]).tobytes()
    assert shapes.tobytes() == np.concatenate([x for _, _, x in got]).tobytes()
    assert (labels == np.stack([t.labels for t, _, _ in got])).all()


def test_torch_mirror_reuses_out_and_refuses_wrong_shapes(torch, eng):
    shape = (4, 126, 94)
    imgs = [cases.smooth_field(shape[1], shape[2], 5100 + k) for k in range(shape[0])]
    lists = [np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2) for im in imgs]
    wt = bc.weight_cubes(shape, 53)[1][1]
    d_wt = _wt_dev(torch, eng, wt)
    cube, seeds, offs = _inputs(torch, eng, imgs, lists)
    total = _first(offs)[-1]
    out = torch.full((total, 4), -7, dtype=torch.int32, device=eng.device)
    out_stats = torch.full((total, 9), -7, dtype=torch.int64, device=eng.device)
    out_shapes = torch.full((total, 12), -7, dtype=torch.int64, device=eng.device)
    tree, stats, shapes, labels = eng.merge_tree_shapes_batch(cube, seeds, offs, weights=d_wt, edge=True, want_labels=True, out=out,
                                                              out_stats=out_stats, out_shapes=out_shapes)
    assert tree.data_ptr() == out.data_ptr() and stats.data_ptr() == out_stats.data_ptr() and shapes.data_ptr() == out_shapes.data_ptr()
    assert tuple(shapes.shape) == (total, 12) and shapes.dtype == torch.int64 and tuple(labels.shape) == (4, 128, 96)
    _check_against_stats_batch_and_single_calls(torch, eng, cube, seeds, offs, wt, (tree, stats, shapes), labels, edge=True)
    again = eng.merge_tree_shapes_batch(cube, seeds, offs, weights=d_wt, edge=True, out=out, out_stats=out_stats, out_shapes=out_shapes)
    assert again[2].data_ptr() == out_shapes.data_ptr()
    with pytest.raises(ValueError):
        eng.merge_tree_shapes_batch(cube, seeds, offs, out=torch.empty((total + 1, 4), dtype=torch.int32, device=eng.device))
    with pytest.raises(ValueError):
        eng.merge_tree_shapes_batch(cube, seeds, offs, out_stats=torch.empty((total, 8), dtype=torch.int64, device=eng.device))
    with pytest.raises(ValueError):
        eng.merge_tree_shapes_batch(cube, seeds, offs, out_shapes=torch.empty((total, 6), dtype=torch.int64, device=eng.device))
    with pytest.raises(ValueError):
        eng.merge_tree_shapes_batch(cube, seeds, offs, out_shapes=torch.empty((total, 12), dtype=torch.int32, device=eng.device))
    with pytest.raises(ValueError):
        eng.merge_tree_shapes_batch(cube, seeds, offs, weights=d_wt[:, :, :90])
    with pytest.raises(TypeError):
        eng.merge_tree_shapes_batch(cube, seeds, offs, weights=d_wt.to(torch.float32))


def test_stack_is_taken_at_size(torch, eng):
    s, h, w = 16, 1024, 1024
    cube = torch.stack([eng.random_field(h, w, 5200 + k) for k in range(s)]).contiguous()
    lists = [eng.find_local_minima(cube[k]) for k in range(s)]
    offs = [0] + [int(x) for x in np.cumsum([int(l.shape[0]) for l in lists])]
    seeds = torch.cat(lists).contiguous()
    g = torch.Generator(device="cpu").manual_seed(52)
    d_wt = torch.randint(-32768, 32768, (s, h, w), generator=g, dtype=torch.int16).to(eng.device)      # u16 bits
    tree, stats, shapes = eng.merge_tree_shapes_batch(cube, seeds, offs, weights=d_wt)
    batch_relax = eng.stats()["launches_relax"]
    first = _first(offs)
    loop_relax = 0
    for k in range(s):
        one = eng.merge_tree_shapes(cube[k], lists[k], weights=d_wt[k])
        loop_relax += eng.stats()["launches_relax"]
        rows = slice(first[k], first[k + 1])
        assert torch.equal(tree[rows], one[0]) and torch.equal(stats[rows], one[1]) and torch.equal(shapes[rows], one[2]), k
    assert batch_relax < loop_relax, (batch_relax, loop_relax)      # one stacked flood, not sixteen
