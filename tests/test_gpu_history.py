"""transform_history for chosen levels (ws_transform_history_device, ws_transform_history) against the CPU oracle's hook
snapshots and the existing hook route (ws_segment_with_hook / ws_merge_with_hook), -m gpu."""
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
def eng(pkg):
    import torch
    with torch.cuda.stream(torch.cuda.Stream(0)):      # a stream of its own: the level loops are captured and replayed
        yield importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


def _ws(pkg, merging, max_level=254, edge=False):
    b = pkg.TransformBuilder.new().set_max_water_lvl(max_level)
    if edge:
        b.enable_edge_correction()
    return b.build_merging() if merging else b.build_segmenting()


def _oracle_levels(img, seeds, merging, **kw):
    snaps = []
    if merging:
        ol.merge(img, seeds, hook=lambda l, m, i, c: snaps.append(ol.canonicalise(c, seeds)[0]), **kw)
    else:
        ol.segment(img, seeds, hook=lambda l, m, i, c: snaps.append(c.copy()), **kw)
    return snaps


def _device_planes(eng, img, seeds, merging, levels=None, max_level=254, edge=False):
    import torch
    t_img = torch.from_numpy(np.ascontiguousarray(img)).to(eng.device)
    t_seeds = torch.from_numpy(np.asarray(seeds, dtype=np.int64).reshape(-1, 2).astype(np.int32)).to(eng.device)
    out = eng.transform_history(t_img, t_seeds, levels=levels, merging=merging, max_level=max_level, edge=edge)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).astype(np.uint64)


@pytest.mark.parametrize("merging", [False, True])
@pytest.mark.parametrize("shape,seed,edge", [((24, 24), 1, False), ((50, 70), 2, False), ((96, 96), 3, True),
                                              ((130, 67), 4, False), ((200, 300), 5, True)])
def test_history_matches_oracle_and_hook_route_every_level(pkg, eng, merging, shape, seed, edge):
    img = cases.field(*shape, seed)
    seeds = ol.find_local_minima(img)
    want = _oracle_levels(img, seeds, merging, edge=edge)
    ws = _ws(pkg, merging, edge=edge)
    hook = ws.transform_history(img, seeds)
    host = ws.transform_history_levels(img, seeds)
    dev = _device_planes(eng, img, seeds, merging, edge=edge)
    assert [l for l, _ in host] == [l for l, _ in hook] == list(range(255))
    assert dev.shape == (255,) + want[0].shape
    for lvl in range(255):
        assert (host[lvl][1] == want[lvl]).all(), lvl
        assert (host[lvl][1] == hook[lvl][1]).all(), lvl
        assert (dev[lvl] == hook[lvl][1]).all(), lvl


@pytest.mark.parametrize("merging", [False, True])
def test_history_adversarial_cases(pkg, eng, merging):
    for name, img, seeds in cases.adversarial_cases():
        seeds = cases.seeds_or_maxima(img, seeds)
        for edge in (False, True):
            want = _oracle_levels(img, seeds, merging, edge=edge)
            got = _ws(pkg, merging, edge=edge).transform_history_levels(img, seeds)
            dev = _device_planes(eng, img, seeds, merging, edge=edge)
            for lvl in range(255):
                assert (got[lvl][1] == want[lvl]).all(), (name, edge, lvl)
                assert (dev[lvl] == want[lvl]).all(), (name, edge, lvl)


@pytest.mark.parametrize("merging", [False, True])
@pytest.mark.parametrize("maxlvl", [1, 60, 254])
def test_history_max_water_level(pkg, eng, merging, maxlvl):
    img = cases.smooth_field(90, 110, 8)
    seeds = ol.find_local_minima(img)
    want = _oracle_levels(img, seeds, merging, max_level=maxlvl)
    assert len(want) == maxlvl + 1
    got = _ws(pkg, merging, max_level=maxlvl).transform_history_levels(img, seeds)
    dev = _device_planes(eng, img, seeds, merging, max_level=maxlvl)
    assert [l for l, _ in got] == list(range(maxlvl + 1)) and dev.shape[0] == maxlvl + 1
    for lvl in range(maxlvl + 1):
        assert (got[lvl][1] == want[lvl]).all(), lvl
        assert (dev[lvl] == want[lvl]).all(), lvl


@pytest.mark.parametrize("merging", [False, True])
def test_level_lists_any_order_repeats_single_and_zero(pkg, eng, merging):
    img = cases.field(77, 64, 12)
    seeds = ol.find_local_minima(img)
    ws = _ws(pkg, merging)
    full = ws.transform_history(img, seeds)
    for levels in ([200, 3, 117, 3, 0, 254, 40], [131], [0], [254, 254]):
        got = ws.transform_history_levels(img, seeds, levels)
        dev = _device_planes(eng, img, seeds, merging, levels=levels)
        assert [l for l, _ in got] == levels
        for k, lvl in enumerate(levels):
            assert (got[k][1] == full[lvl][1]).all(), (levels, k)
            assert (dev[k] == full[lvl][1]).all(), (levels, k)


def _raw(pkg, eng, img, seeds, levels, out, plane_stride, merging=1, max_level=254):
    """ws_transform_history_device itself (the Python wrapper refuses bad lists before the library sees them)."""
    import torch
    opt = eng.options(max_level)
    lv = np.asarray(levels, dtype=np.uint8)
    h, w = img.shape
    rc = pkg._ffi.lib().ws_transform_history_device(eng.ctx.handle, merging, img.data_ptr(), h, w, w,
                                                     seeds.data_ptr() if seeds.numel() else None, seeds.shape[0], ctypes.byref(opt),
                                                     lv.ctypes.data if lv.size else None, lv.size, out.data_ptr(), plane_stride)
    torch.cuda.synchronize()
    return rc


def test_no_levels_writes_nothing_and_gaps_stay_untouched(pkg, eng):
    import torch
    img = eng.random_field(40, 52, 3)
    seeds = eng.find_local_minima(img)
    n = 40 * 52
    sentinel = 0x5A5A5A5A
    buf = torch.full((3 * (n + 37),), sentinel, dtype=torch.int32, device=eng.device)
    assert _raw(pkg, eng, img, seeds, [], buf, n + 37) == 0
    assert bool((buf == sentinel).all())
    levels = [90, 5, 254]
    assert _raw(pkg, eng, img, seeds, levels, buf, n + 37) == 0
    want = eng.transform_history(img, seeds, levels=levels, merging=True)
    planes = buf.view(3, n + 37)
    assert bool((planes[:, n:] == sentinel).all())                 # the gaps between the planes
    assert bool((planes[:, :n].reshape(3, 40, 52) == want).all())


def test_bad_levels_and_short_stride_are_refused(pkg, eng):
    import torch
    bad = pkg._ffi.WS_ERR_BAD_ARG
    img = eng.random_field(32, 32, 4)
    seeds = eng.find_local_minima(img)
    buf = torch.full((4 * 1024,), 7, dtype=torch.int32, device=eng.device)
    assert _raw(pkg, eng, img, seeds, [3, 61], buf, 1024, max_level=60) == bad
    assert _raw(pkg, eng, img, seeds, [255], buf, 1024) == bad
    assert _raw(pkg, eng, img, seeds, [1, 2], buf, 1023) == bad
    assert _raw(pkg, eng, img, seeds, [], buf, 1023) == bad          # (no levels: still a short stride)
    assert _raw(pkg, eng, img, seeds, list(range(200)) + list(range(57)), torch.empty((257 * 1024,), dtype=torch.int32, device=eng.device), 1024) == bad
    assert bool((buf == 7).all())                                   # refused before anything ran


@pytest.mark.parametrize("merging", [False, True])
def test_empty_images_and_seedless_planes_give_zero_planes(pkg, eng, merging):
    ws = _ws(pkg, merging)
    got = ws.transform_history_levels(np.full((30, 40), 9, np.uint8), np.zeros((0, 2), np.uint64), [0, 100, 254])
    assert len(got) == 3 and all(p.shape == (30, 40) and not p.any() for _, p in got)
    dev = _device_planes(eng, np.full((30, 40), 9, np.uint8), np.zeros((0, 2)), merging, levels=[0, 254])
    assert dev.shape == (2, 30, 40) and not dev.any()
    got = _ws(pkg, merging, edge=True).transform_history_levels(np.zeros((0, 0), np.uint8), np.zeros((0, 2), np.uint64), [0, 7])
    assert len(got) == 2 and all(p.shape == (2, 2) and not p.any() for _, p in got)
    got = ws.transform_history_levels(np.zeros((0, 5), np.uint8), np.zeros((0, 2), np.uint64), [4])
    assert len(got) == 1 and got[0][1].shape == (0, 5)


def test_graph_keys_keep_history_lists_and_final_labels_apart(pkg, eng):
    # merge_host captures its level loop on the second of two calls with the same key in a row and replays it from then on.  Every
    # kind of call below runs three times in a row on ONE context, so that its loop is captured and then replayed, before the next
    # kind takes over: history (device form), the hookless ws_merge_with_hook, history again, history through the host form, the
    # hookless merge again, transform_to_list_device, history again.  The hookless merge and history have keys that differ in
    # nothing but the history flag (same planes, no record buffer): a hookless graph replayed for history would leave the merge
    # forest unstamped and every merging plane would show segmenting colours -- and the reverse would replay history's unions.
    import torch
    L = pkg._ffi.lib()
    h, w = 300, 260
    img = eng.random_field(h, w, 21)
    seeds = eng.find_local_minima(img)
    himg = img.cpu().numpy()
    hseeds = seeds.cpu().numpy().astype(np.uint64)
    levels = [254, 0, 77, 160, 121]
    hook = _ws(pkg, True).transform_history(himg, hseeds)          # (the default context: a reference of its own)
    want_hist = np.stack([hook[lvl][1] for lvl in levels]).astype(np.uint32)
    want_final = hook[254][1]
    areas = np.bincount(want_final.ravel().astype(np.int64))
    want_records = sorted((int(c), int(a)) for c, a in enumerate(areas) if c and a)
    assert not (want_hist[0] == want_hist[2]).all()                  # the planes do differ from level to level
    host_ws = pkg.TransformBuilder.new().set_context(eng.ctx).build_merging()
    opt = eng.options(254)
    out64 = np.empty((h, w), dtype=np.uint64)

    def history_device():
        got = eng.transform_history(img, seeds, levels=levels, merging=True)
        torch.cuda.synchronize()
        return (got.cpu().numpy().view(np.uint32) == want_hist).all()

    def history_host():
        got = host_ws.transform_history_levels(himg, hseeds, levels)
        return (np.stack([p for _, p in got]) == want_hist).all()

    def hookless_merge():
        eng.ctx.check(L.ws_merge_with_hook(eng.ctx.handle, himg.ctypes.data, h, w, w, hseeds.ctypes.data, hseeds.shape[0],
                                           ctypes.byref(opt), None, None, out64.ctypes.data))
        return (out64 == want_final).all()

    def to_list():
        lakes, off, _ = eng.transform_to_list(img, seeds, merging=True)
        torch.cuda.synchronize()
        rec = lakes.cpu().numpy()[int(off[254]):int(off[255])]
        return sorted(map(tuple, rec.tolist())) == want_records

    groups = (255 + 15) // 16                                       # the level loop's graphs: one per 16 levels
    sequence = [history_device, hookless_merge, history_device, history_host, hookless_merge, to_list, history_device]
    for k, fn in enumerate(sequence):
        for i in range(3):
            assert fn(), (k, fn.__name__, i)
            launches = eng.ctx.stats()["graph_launches"]
            # history after a call that was not one (or the reverse): nothing of the previous kind's graphs is replayed.  (The
            # two history forms share their graphs: same kernels, same buffers.)
            if i == 0 and k > 0 and ("history" in fn.__name__) != ("history" in sequence[k - 1].__name__):
                assert launches < groups, (k, fn.__name__, launches)
            if i == 2:                # captured by the second call, replayed by the third: every group a graph launch
                assert launches >= groups, (k, fn.__name__, launches)


def test_history_4096_many_colours_equals_hook_route(pkg, eng):
    import torch
    size = 4096
    img = eng.random_field(size, size, 9)
    seeds = eng.find_local_minima(img)
    assert seeds.shape[0] > 1_500_000
    levels = [0, 1, 40, 100, 120, 125, 130, 200, 254]
    dev = eng.transform_history(img, seeds, levels=levels, merging=True)
    torch.cuda.synchronize()
    b = pkg.TransformBuilder.new()
    keep = {}
    b.set_wlvl_hook(lambda ctx: keep.__setitem__(ctx.water_level, ctx.colours.astype(np.uint32)) if ctx.water_level in levels else None)
    b.build_merging().transform_with_hook(img.cpu().numpy(), seeds.cpu().numpy().astype(np.uint64))
    assert sorted(keep) == sorted(set(levels))
    got = dev.cpu().numpy().view(np.uint32)
    for k, lvl in enumerate(levels):
        assert (got[k] == keep[lvl]).all(), lvl


@pytest.mark.parametrize("merging", [False, True])
def test_history_8192_bench_field(pkg, eng, merging):
    import torch
    size = 8192
    img = eng.random_field(size, size, 1)
    seeds = eng.find_local_minima(img)
    levels = [0, 64, 128, 254]
    hist = eng.transform_history(img, seeds, levels=levels, merging=merging)
    if merging:
        fin = eng.merge(img, seeds)
        assert bool((hist[3] == fin).all())
    else:
        lab = eng.segment(img, seeds)
        for k, lvl in enumerate(levels):
            assert bool((hist[k] == eng.level_snapshot(lab, lvl)).all()), lvl
    torch.cuda.synchronize()
    ncol = seeds.shape[0] + 1
    for k in range(3):      # the coloured set grows; every lake of level k lies inside one lake of level k + 1
        a = hist[k].flatten().to(torch.int64)
        b = hist[k + 1].flatten().to(torch.int64)
        assert bool(((a == 0) | (b != 0)).all()), levels[k]
        m = a != 0
        to = torch.full((ncol,), -1, dtype=torch.int64, device=a.device)
        to.scatter_(0, a[m], b[m])
        assert bool((to[a[m]] == b[m]).all()), levels[k]
        del a, b, m, to


def test_host_form_spans_several_chunks(pkg):
    # 255 planes of 1024 x 600 u32 are 627 MB: three chunks of the host form's 256 MiB scratch, each crossing the bus as u32 words
    # widened by the host threads; without host threads (and for small chunks) the planes cross one by one, widened on the device
    img = cases.field(1024, 600, 31)
    seeds = ol.find_local_minima(img)
    L = pkg._ffi.lib()
    plain = pkg.api.Context(0)
    assert L.ws_ctx_set_host_threads(plain.handle, 0) == 0
    for merging in (False, True):
        ws = _ws(pkg, merging)
        got = ws.transform_history_levels(img, seeds)
        want = ws.transform_history(img, seeds)
        assert len(got) == len(want) == 255
        for (lg, pg), (lw, pw) in zip(got, want):
            assert lg == lw and (pg == pw).all(), (merging, lg)
        b = pkg.TransformBuilder.new().set_context(plain)
        levels = [254, 0, 130, 0]
        out = np.full((4, 1024, 600), 7, dtype=np.uint64)
        planes = (b.build_merging() if merging else b.build_segmenting()).transform_history_levels(img, seeds, levels, out=out)
        for k, (lvl, p) in enumerate(planes):
            assert lvl == levels[k] and p.base is out and (out[k] == want[lvl][1]).all(), (merging, k)
        del got, want
    plain.close()


def test_torch_mirror_matches_level_snapshot_and_hook_route(pkg, eng):
    import torch
    img = eng.random_field(256, 320, 17)
    seeds = eng.find_local_minima(img)
    lab = eng.segment(img, seeds)
    levels = [3, 250, 0, 120]
    seg = eng.transform_history(img, seeds, levels=levels)
    for k, lvl in enumerate(levels):
        assert bool((seg[k] == eng.level_snapshot(lab, lvl)).all()), lvl
    mer = eng.transform_history(img, seeds, levels=levels, merging=True)
    torch.cuda.synchronize()
    hook = _ws(pkg, True).transform_history(img.cpu().numpy(), seeds.cpu().numpy().astype(np.uint64))
    got = mer.cpu().numpy().view(np.uint32)
    for k, lvl in enumerate(levels):
        assert (got[k] == hook[lvl][1]).all(), lvl
    # the stamps of this transform stay readable afterwards
    assert eng.last_arrival().shape == (256, 320)
