"""transform_history of a cube of slices in one call (ws_transform_history_batch(_device)), on the GPU: every (slice, level) plane
against ws_transform_history_device on that slice alone and the CPU oracle's hook snapshots, the stack's own guarantees (it is
taken, groups, failing slice, graph keys on a shared context) and the host form's chunks."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import cases
import oracle_lib as ol

pytestmark = pytest.mark.gpu


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


def _ws(pkg, merging, max_level=254, edge=False, ctx=None):
    b = pkg.TransformBuilder.new().set_max_water_lvl(max_level)
    if edge:
        b.enable_edge_correction()
    if ctx is not None:
        b.set_context(ctx)
    return b.build_merging() if merging else b.build_segmenting()


def _seed_lists(imgs):
    """The slices' own minima, except: slice 1 has no seed, slice 2 a single one."""
    lists = [np.asarray(ol.find_local_minima(im), dtype=np.int64).reshape(-1, 2) for im in imgs]
    lists[1] = lists[1][:0]
    lists[2] = lists[2][:1]
    return lists


def _device_inputs(torch, eng, imgs, lists):
    flat = np.concatenate(lists, axis=0) if sum(len(l) for l in lists) else np.zeros((0, 2), np.int64)
    offs = [0] + [int(x) for x in np.cumsum([len(l) for l in lists])]
    cube = torch.from_numpy(np.stack(imgs)).to(eng.device).contiguous()
    return cube, torch.from_numpy(flat.astype(np.int32)).to(eng.device).contiguous(), offs


def _oracle_levels(img, seeds, merging, **kw):
    snaps = []
    s = [tuple(map(int, p)) for p in seeds]
    if merging:
        ol.merge(img, s, hook=lambda l, m, i, c: snaps.append(ol.canonicalise(c, s)[0]), **kw)
    else:
        ol.segment(img, s, hook=lambda l, m, i, c: snaps.append(c.copy()), **kw)
    return snaps


def _raw_device(pkg, eng, cube, seeds, offs, levels, out, plane_stride, merging=1, max_level=254, edge=False, failed=None):
    """ws_transform_history_batch_device itself (the wrappers refuse bad lists before the library sees them)."""
    import torch
    s, h, w = cube.shape
    opt = eng.options(max_level, edge)
    lv = np.asarray(levels, dtype=np.uint8)
    c_offs = (ctypes.c_size_t * (s + 1))(*[int(x) for x in offs])
    rc = pkg._ffi.lib().ws_transform_history_batch_device(eng.ctx.handle, merging, cube.data_ptr(), s, h, w, w, h * w,
                                                          seeds.data_ptr() if seeds.numel() else None, c_offs, ctypes.byref(opt),
                                                          lv.ctypes.data if lv.size else None, lv.size, out.data_ptr(), plane_stride,
                                                          ctypes.byref(failed) if failed is not None else None)
    torch.cuda.synchronize()
    return rc


SHAPES = [((6, 128, 96), False), ((6, 126, 94), True),      # stack: the plane (padded with edge correction) is 128 x 96
          ((5, 130, 98), False), ((5, 130, 98), True)]      # no stack: w' % 4 != 0


@pytest.mark.parametrize("merging", [True, False])
@pytest.mark.parametrize("max_level,levels", [(254, None), (90, [90, 3, 17, 3, 0])])
@pytest.mark.parametrize("shape,edge", SHAPES)
def test_history_batch_matches_single_calls_and_oracle_per_slice(pkg, torch, merging, max_level, levels, shape, edge):
    s, h, w = shape
    eng = _engine(pkg)
    imgs = [cases.field(h, w, 1100 + 7 * k) for k in range(s)]
    lists = _seed_lists(imgs)
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    got = eng.transform_history_batch(cube, seeds, offs, levels=levels, merging=merging, max_level=max_level, edge=edge)
    lv = list(range(max_level + 1)) if levels is None else levels
    e = 2 if edge else 0
    assert tuple(got.shape) == (s, len(lv), h + e, w + e)
    got = got.cpu().numpy().view(np.uint32)
    for k in range(s):
        one = eng.transform_history(cube[k], seeds[offs[k]:offs[k + 1]], levels=levels, merging=merging, max_level=max_level, edge=edge)
        one = one.cpu().numpy().view(np.uint32)
        want = _oracle_levels(imgs[k], lists[k], merging, max_level=max_level, edge=edge) if len(lists[k]) else None
        for j, lvl in enumerate(lv):
            assert (got[k, j] == one[j]).all(), (shape, edge, merging, k, lvl)
            if want is not None:
                assert len(want) == max_level + 1
                assert (got[k, j].astype(np.uint64) == want[lvl]).all(), (shape, edge, merging, k, lvl)
        if k == 1:
            assert not got[k].any()                                  # the seedless slice


@pytest.mark.parametrize("merging", [1, 0])
@pytest.mark.parametrize("shape", [(6, 128, 96), (5, 130, 98)])
def test_level_lists_and_untouched_gaps(pkg, torch, merging, shape):
    s, h, w = shape
    n = h * w
    eng = _engine(pkg)
    imgs = [cases.field(h, w, 1200 + k) for k in range(s)]
    lists = _seed_lists(imgs)
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    full = eng.transform_history_batch(cube, seeds, offs, merging=bool(merging)).cpu().numpy()      # every level, in order
    sentinel = 0x5A5A5A5A
    for gap in (64, 37):      # a stride that keeps the 16-byte stores, and one that does not
        stride = n + gap
        buf = torch.full((s * 8 * stride,), sentinel, dtype=torch.int32, device=eng.device)
        assert _raw_device(pkg, eng, cube, seeds, offs, [], buf, stride, merging) == 0
        assert bool((buf == sentinel).all())                       # nothing asked, nothing written
        for levels in ([200, 3, 117, 3, 0, 254, 40], [131], [254, 254]):
            buf.fill_(sentinel)
            assert _raw_device(pkg, eng, cube, seeds, offs, levels, buf, stride, merging) == 0
            k_n = len(levels)
            planes = buf[: s * k_n * stride].view(s * k_n, stride).cpu().numpy()
            assert (planes[:, n:] == sentinel).all(), (gap, levels)           # the gaps between the planes
            assert (buf[s * k_n * stride:] == sentinel).all().item(), (gap, levels)
            for k in range(s):
                for j, lvl in enumerate(levels):
                    assert (planes[k * k_n + j, :n].reshape(h, w) == full[k, lvl]).all(), (gap, levels, k, j)


def test_bad_levels_and_short_stride_are_refused(pkg, torch):
    eng = _engine(pkg)
    bad = pkg._ffi.WS_ERR_BAD_ARG
    s, h, w = 3, 32, 32
    imgs = [cases.field(h, w, 1300 + k) for k in range(s)]
    cube, seeds, offs = _device_inputs(torch, eng, imgs, [np.asarray(ol.find_local_minima(im), np.int64).reshape(-1, 2) for im in imgs])
    buf = torch.full((s * 4 * 1024,), 7, dtype=torch.int32, device=eng.device)
    assert _raw_device(pkg, eng, cube, seeds, offs, [3, 61], buf, 1024, max_level=60) == bad
    assert _raw_device(pkg, eng, cube, seeds, offs, [255], buf, 1024) == bad
    assert _raw_device(pkg, eng, cube, seeds, offs, [1, 2], buf, 1023) == bad
    assert _raw_device(pkg, eng, cube, seeds, offs, [], buf, 1023) == bad
    big = torch.empty((s * 257 * 1024,), dtype=torch.int32, device=eng.device)
    assert _raw_device(pkg, eng, cube, seeds, offs, list(range(200)) + list(range(57)), big, 1024) == bad
    assert bool((buf == 7).all())                                   # refused before anything ran


def test_stack_is_taken_at_size(pkg, torch):
    s, h, w = 16, 1024, 1024
    eng = _engine(pkg)
    cube = torch.stack([eng.random_field(h, w, 1400 + k) for k in range(s)]).contiguous()
    lists = [eng.find_local_minima(cube[k]) for k in range(s)]
    offs = [0] + [int(x) for x in np.cumsum([int(l.shape[0]) for l in lists])]
    seeds = torch.cat(lists).contiguous()
    levels = [0, 100, 254, 180]
    for merging in (True, False):
        got = eng.transform_history_batch(cube, seeds, offs, levels=levels, merging=merging)
        batch_relax = eng.stats()["launches_relax"]
        loop_relax = 0
        for k in range(s):
            one = eng.transform_history(cube[k], lists[k], levels=levels, merging=merging)
            loop_relax += eng.stats()["launches_relax"]
            assert torch.equal(got[k], one), (merging, k)
        assert batch_relax < loop_relax, (merging, batch_relax, loop_relax)      # one stacked flood, not sixteen
        del got


@pytest.mark.parametrize("merging", [True, False])
def test_several_groups_equal_one(pkg, torch, merging):
    s, h, w = 7, 128, 96
    eng = _engine(pkg)
    imgs = [cases.field(h, w, 1500 + k) for k in range(s)]
    lists = [np.asarray(ol.find_local_minima(im), np.int64).reshape(-1, 2) for im in imgs]
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    levels = [254, 0, 60, 130]
    one_group = eng.transform_history_batch(cube, seeds, offs, levels=levels, merging=merging)
    one_relax = eng.stats()["launches_relax"]
    eng.ctx.set_batch_pixel_limit(3 * h * w)                        # 3 + 3 + 1 slices
    try:
        groups = eng.transform_history_batch(cube, seeds, offs, levels=levels, merging=merging)
        groups_relax = eng.stats()["launches_relax"]
    finally:
        eng.ctx.set_batch_pixel_limit(0)
    assert torch.equal(groups, one_group)
    assert groups_relax > one_relax                                 # three floods, not one
    for k in (0, 4, 6):
        assert torch.equal(groups[k], eng.transform_history(cube[k], seeds[offs[k]:offs[k + 1]], levels=levels, merging=merging)), k


@pytest.mark.parametrize("shape", [(6, 128, 96), (5, 130, 98)])
def test_failing_slice_is_named(pkg, torch, shape):
    s, h, w = shape
    eng = _engine(pkg)
    imgs = [cases.field(h, w, 1600 + k) for k in range(s)]
    for bad_k in (3, 0):
        lists = [np.asarray(ol.find_local_minima(im), np.int64).reshape(-1, 2) for im in imgs]
        lists[bad_k] = np.concatenate([lists[bad_k], np.array([[4000, 3]], np.int64)])
        cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
        out = torch.empty((s * 2 * h * w,), dtype=torch.int32, device=eng.device)
        failed = ctypes.c_size_t(99)
        rc = _raw_device(pkg, eng, cube, seeds, offs, [10, 254], out, h * w, failed=failed)
        assert rc == pkg._ffi.WS_ERR_SEED_OOB and failed.value == bad_k, (shape, bad_k, rc, failed.value)
    # ... and the context works on
    lists = [np.asarray(ol.find_local_minima(im), np.int64).reshape(-1, 2) for im in imgs]
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    got = eng.transform_history_batch(cube, seeds, offs, levels=[254], merging=True).cpu().numpy().astype(np.uint64)
    assert (got[s - 1, 0] == _oracle_levels(imgs[s - 1], lists[s - 1], True)[254]).all()


def test_history_lists_single_and_merge_batches_alternate_on_one_context(pkg, torch, stream):
    # merge_host captures its level loop on the second of two calls with the same key in a row and replays it from then on.  On
    # ONE context, each of four kinds of call in turn, three rounds: the stacked history loop (stamping unions over the stack's
    # colours), the stacked list loop, the single-field history loop and the merge batch.  A graph replayed for the wrong kind
    # would leave the forest unstamped, or stamp it in another numbering, and a plane or a record set would change.
    eng = _engine(pkg)
    L = pkg._ffi.lib()
    s, h, w = 4, 128, 96
    imgs = [cases.field(h, w, 1700 + k) for k in range(s)]
    lists = [np.asarray(ol.find_local_minima(im), np.int64).reshape(-1, 2) for im in imgs]
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    levels = [254, 0, 77, 160, 121]
    first = {}

    def history_batch():
        return eng.transform_history_batch(cube, seeds, offs, levels=levels, merging=True).clone()

    def list_batch():      # (records within a (slice, level) come in no particular order: compared as sorted keys)
        lakes, offsets, unc = eng.transform_to_list_batch(cube, seeds, offs, merging=True)
        counts = torch.from_numpy(np.diff(offsets.astype(np.int64))).to(lakes.device)
        b = torch.repeat_interleave(torch.arange(counts.numel(), device=lakes.device, dtype=torch.int64), counts)
        return torch.sort((b << 40) | (lakes[:, 0] << 20) | lakes[:, 1]).values, offsets.copy(), unc.copy()

    def single_history():
        return eng.transform_history(cube[2], seeds[offs[2]:offs[3]], levels=levels, merging=True).clone()

    def merge_batch():
        return eng.merge_batch(cube, seeds, offs).clone()

    def same(a, b):
        if isinstance(a, tuple):
            return torch.equal(a[0], b[0]) and (a[1] == b[1]).all() and (a[2] == b[2]).all()
        return torch.equal(a, b)

    want_hist = np.stack([np.stack([p for p in _oracle_levels(imgs[k], lists[k], True)]) for k in range(s)])[:, levels]
    for rep in range(3):
        for fn in (history_batch, list_batch, single_history, merge_batch):
            for i in range(3):
                got = fn()
                torch.cuda.synchronize()
                if fn.__name__ not in first:
                    first[fn.__name__] = got
                assert same(got, first[fn.__name__]), (rep, fn.__name__, i)
                if fn is history_batch:
                    assert (got.cpu().numpy().astype(np.uint64) == want_hist).all(), (rep, i)
                    if i == 2:      # captured by the second call, replayed by the third: every group of 16 levels a graph launch
                        assert eng.stats()["graph_launches"] >= 16, (rep, eng.stats()["graph_launches"])
                    p = ctypes.c_void_p()
                    hh, ww = ctypes.c_size_t(), ctypes.c_size_t()
                    assert L.ws_last_arrival_device(eng.ctx.handle, ctypes.byref(p), ctypes.byref(hh), ctypes.byref(ww)) == \
                        pkg._ffi.WS_ERR_UNSUPPORTED
    assert (first["single_history"].cpu().numpy().astype(np.uint64) == want_hist[2]).all()


@pytest.mark.parametrize("merging", [True, False])
@pytest.mark.parametrize("shape", [(5, 128, 112), (5, 130, 98)])      # a stack, and the loop
def test_host_form_equals_slice_calls(pkg, merging, shape):
    s, h, w = shape
    cube = np.stack([cases.field(h, w, 1800 + k) for k in range(s)])
    ws = _ws(pkg, merging, max_level=200)
    levels = [200, 0, 33, 33, 150]
    mins = [ws.find_local_minima(cube[k]) for k in range(s)]
    got, counts = ws.transform_history_cube(cube, levels=levels)
    given = ws.transform_history_cube(cube, seeds=mins, levels=levels)
    assert len(got) == len(given) == s
    for k in range(s):
        assert counts[k] == len(mins[k])
        want = ws.transform_history_levels(cube[k], mins[k], levels)
        for (lg, pg), (lh, ph), (lw, pw) in zip(got[k], given[k], want):
            assert lg == lh == lw and (pg == pw).all() and (ph == pw).all(), (k, lw)
    # every level, an out array reused
    out = np.full((s, 201, h, w), 3, dtype=np.uint64)
    allp = ws.transform_history_cube(cube, seeds=mins, out=out)
    for k in (0, 4):
        hook = ws.transform_history(cube[k], mins[k])
        for (lg, pg), (lw, pw) in zip(allp[k], hook):
            assert lg == lw and pg.base is out and (pg == pw).all(), (k, lw)


def test_host_form_spans_several_chunks(pkg):
    # 16 x 1024^2 with 5 levels: 80 planes of 4 MiB in u32, two chunks of whole slices of the 256 MiB scratch (12 + 4 slices),
    # each crossing the bus as ONE copy.  2 x 1024^2 with 65 levels: a slice's planes do not fit, its levels are split.  And the
    # same without host threads: plane by plane, widened on the device.
    L = pkg._ffi.lib()
    plain = pkg.api.Context(0)
    assert L.ws_ctx_set_host_threads(plain.handle, 0) == 0
    cube = np.stack([cases.field(1024, 1024, 1900 + k) for k in range(16)])
    for merging in (True, False):
        for ctx in (None, plain):
            ws = _ws(pkg, merging, ctx=ctx)
            levels = [254, 0, 130, 64, 130]
            got, counts = ws.transform_history_cube(cube, levels=levels)
            for k in range(16):
                mins = ws.find_local_minima(cube[k])
                assert counts[k] == len(mins)
                want = ws.transform_history_levels(cube[k], mins, levels)
                for j in range(len(levels)):
                    assert got[k][j][0] == levels[j] and (got[k][j][1] == want[j][1]).all(), (merging, ctx is None, k, j)
            del got
        ws = _ws(pkg, merging)
        levels = list(range(0, 255, 4)) + [254]
        assert len(levels) == 65
        got, _ = ws.transform_history_cube(cube[:2], levels=levels)
        for k in range(2):
            want = ws.transform_history_levels(cube[k], ws.find_local_minima(cube[k]), levels)
            for j in range(65):
                assert (got[k][j][1] == want[j][1]).all(), (merging, k, j)
            del want
        del got
    plain.close()


def test_torch_mirror_equals_host_form_and_reuses_out(pkg, torch):
    eng = _engine(pkg)
    s, h, w = 4, 126, 94
    imgs = [cases.smooth_field(h, w, 2000 + k) for k in range(s)]
    lists = [np.asarray(ol.find_local_minima(im), np.int64).reshape(-1, 2) for im in imgs]
    cube, seeds, offs = _device_inputs(torch, eng, imgs, lists)
    levels = [5, 250, 0, 120]
    for merging in (True, False):
        out = torch.full((s, len(levels), h + 2, w + 2), -1, dtype=torch.int32, device=eng.device)
        got = eng.transform_history_batch(cube, seeds, offs, levels=levels, merging=merging, edge=True, out=out)
        assert got.data_ptr() == out.data_ptr()
        host = _ws(pkg, merging, edge=True).transform_history_cube(np.stack(imgs), seeds=[l.astype(np.uint64) for l in lists], levels=levels)
        g = got.cpu().numpy().view(np.uint32).astype(np.uint64)
        for k in range(s):
            for j in range(len(levels)):
                assert host[k][j][0] == levels[j] and (g[k, j] == host[k][j][1]).all(), (merging, k, j)
    empty = eng.transform_history_batch(cube, seeds, offs, levels=[])
    assert tuple(empty.shape) == (s, 0, h, w)
