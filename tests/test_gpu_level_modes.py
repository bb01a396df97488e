"""Every product of the per-level driver (merge_host, ws_lists.hip) through every source it exists for, bit for bit against the
CPU oracle, -m gpu: lists (segmenting; merging below and above the live-list threshold), the hook, final labels, history
(segmenting, merging), the tree and the tree with statistics -- from a host image, a device image, the arrival planes of a
finished transform (ws_lists_from_arrival_device) and a stacked batch.  One 48 x 64 random field (uniform in [0, 254),
max_water_level 254, seeds from find_local_minima) and a stack of 3 slices of 32 x 64, with edge correction on and off.

Every device-form call is made three times in a row on a context of its own: the first runs plain launches, the second captures
the level loop, the third replays it; all three results are equal.  graph_launches after the three calls, as recorded on the
library before the driver was split into stages and unchanged since: [0, 16, 16] or [0, 16, 17] for every product with a level
loop (one graph per 16 levels; the 17th is the flood's own graph, which unpadded planes replay), [0, 0, 1] and [0, 0, 0] for the
segmenting history and the final labels of ws_merge_device and ws_merge_batch_device, which have no level loop.  The batch calls
are made three times too: the stack (edge correction off) captures and replays as a single field does; with edge correction on
the padded plane does not stack, the slices run one by one with a different seed count each, so no call repeats the one before
it and nothing is ever captured: [0, 0, 0].  (The lowest threshold ws_ctx_set_live_list_min_colours can set is 1 -- it reads 0
as "restore the default" -- so the live-list form is reached with 1: every seed list here is longer.)"""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import lake_stats_ref as ls
import merge_tree_ref as mt
import oracle_lib as ol

pytestmark = pytest.mark.gpu

H, W, SLICES, SLICE_H, MAXLVL, LEVELS = 48, 64, 3, 32, 254, 255


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


def _engine(pkg, stream):
    return importlib.import_module("rustronomy_watershed_amd.device").DeviceEngine(0)


def _oracle_one(img, seeds, edge):
    """The oracle's products of one field: per-level lake sizes (segmenting, merging) and planes, the tree, the statistics."""
    ref = {"img": img, "seeds": seeds}
    seg_sizes, seg_planes, mer_sizes = [], [], []
    ol.segment(img, seeds, max_level=MAXLVL, edge=edge, hook=lambda l, m, i, c: (seg_sizes.append(ol.find_lake_sizes(c)), seg_planes.append(c.copy())))
    ol.merge_arrival(img, seeds, max_level=MAXLVL, edge=edge, hook=lambda l, m, i, c: mer_sizes.append(ol.find_lake_sizes(c)))
    planes, ps = mt.oracle_planes(img, seeds, MAXLVL, edge)
    parent, death, area, leaves, _vals, ex = mt.tree_from_planes(planes, ps)
    ref.update(seg_sizes=seg_sizes, mer_sizes=mer_sizes, seg_planes=np.stack(seg_planes), mer_planes=np.stack(planes),
               tree=np.stack([parent, death, area, leaves], axis=1).astype(np.uint32),
               stats=ls.stats_from_planes(planes, ps, ls.plane_weights(img, None, edge), death, ex))
    return ref


_REFS = {}


def _ref(edge):
    """Computed once per edge setting, shared by every test, never changed."""
    if edge not in _REFS:
        img = ol.random_field(H, W, 41)
        cube = [ol.random_field(SLICE_H, W, 50 + k) for k in range(SLICES)]
        _REFS[edge] = {"field": _oracle_one(img, ol.find_local_minima(img), edge),
                       "stack": [_oracle_one(s, ol.find_local_minima(s), edge) for s in cube]}
        assert all(len(r["seeds"]) > 1 for r in [_REFS[edge]["field"]] + _REFS[edge]["stack"])
    return _REFS[edge]


def _to_dev(torch, eng, ref):
    img = torch.from_numpy(ref["img"]).to(eng.device)
    seeds = torch.from_numpy(np.asarray(ref["seeds"], dtype=np.int64).reshape(-1, 2).astype(np.int32)).to(eng.device).contiguous()
    return img, seeds


def _stack_to_dev(torch, eng, refs):
    cube = torch.from_numpy(np.stack([r["img"] for r in refs])).to(eng.device).contiguous()
    lists = [np.asarray(r["seeds"], dtype=np.int64).reshape(-1, 2).astype(np.int32) for r in refs]
    offs = [0] + [int(x) for x in np.cumsum([len(l) for l in lists])]
    return cube, torch.from_numpy(np.concatenate(lists)).to(eng.device).contiguous(), offs


def _check_lists(rec, offsets, unc, want, tag, first=0):
    """Records of LEVELS levels starting at bin `first` against the oracle's lake sizes: the same colours with the same areas."""
    rec = np.asarray(rec).astype(np.int64)
    for lvl, w in enumerate(want):
        b = first + lvl
        r = rec[int(offsets[b]):int(offsets[b + 1])]
        nz = np.nonzero(w[1:])[0] + 1
        assert int(unc[b]) == int(w[0]), (tag, lvl, int(unc[b]), int(w[0]))
        assert len(r) == len(nz) and (np.sort(r[:, 0]) == nz).all() and (r[np.argsort(r[:, 0]), 1] == w[nz].astype(np.int64)).all(), (tag, lvl)


def _keyed(rec, off):
    """Every level's records as sorted keys colour << 32 | area: the order inside a level is the order the waves wrote them in."""
    r = rec.cpu().numpy()
    return np.concatenate([np.sort((r[int(off[l]):int(off[l + 1]), 0] << 32) | r[int(off[l]):int(off[l + 1]), 1]) for l in range(len(off) - 1)])


def _records(keyed):
    return np.stack([keyed >> 32, keyed & 0xFFFFFFFF], axis=1)


GROUPS = (LEVELS + 15) // 16      # the level loop's graphs: one per 16 levels


def _thrice(eng, call, tag, level_loop=True):
    """plain, capture, replay on one fresh context: equal results; graph_launches 0 after the first call, every group of levels a
    graph launch in the second and third -- or, without a level loop, never as many as that."""
    results, launches = [], []
    for _ in range(3):
        results.append(call())
        launches.append(eng.stats()["graph_launches"])
    print(tag, "graph_launches", launches)
    for got in results[1:]:
        assert len(got) == len(results[0]) and all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(got, results[0])), tag
    assert launches[0] == 0, (tag, launches)
    assert (min(launches[1:]) >= GROUPS) if level_loop else (max(launches) < GROUPS), (tag, launches)
    return results[2]


def _live(pkg, eng, live):
    if live:
        assert pkg._ffi.lib().ws_ctx_set_live_list_min_colours(eng.ctx.handle, 1) == 0


# (merging, live): segmenting; merging with the threshold at its default; merging with the threshold lowered
LIST_MODES = [(False, False), (True, False), (True, True)]


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("merging,live", LIST_MODES)
def test_lists_host_device_arrival(pkg, torch, stream, merging, live, edge):
    ref = _ref(edge)["field"]
    want = ref["mer_sizes"] if merging else ref["seg_sizes"]
    tag = ("lists", merging, live, edge)
    # host
    host_ctx = pkg.api.Context(0)
    if live:
        assert pkg._ffi.lib().ws_ctx_set_live_list_min_colours(host_ctx.handle, 1) == 0
    b = pkg.TransformBuilder.new().set_max_water_lvl(MAXLVL).set_context(host_ctx)
    if edge:
        b.enable_edge_correction()
    sparse = (b.build_merging() if merging else b.build_segmenting()).transform_to_list_sparse(ref["img"], ref["seeds"])
    assert [l for l, *_ in sparse] == list(range(LEVELS))
    for (lvl, unc, colours, areas), w in zip(sparse, want):
        nz = np.nonzero(w[1:])[0] + 1
        order = np.argsort(colours)
        assert unc == int(w[0]) and (colours[order] == nz).all() and (areas[order] == w[nz]).all(), (tag, "host", lvl)
    host_ctx.close()
    # device, three times into one record buffer
    eng = _engine(pkg, stream)
    _live(pkg, eng, live)
    img, seeds = _to_dev(torch, eng, ref)
    lakes = torch.zeros((LEVELS * (len(ref["seeds"]) + 1), 2), dtype=torch.int64, device=eng.device)

    def device():
        rec, off, unc = eng.transform_to_list(img, seeds, merging=merging, max_level=MAXLVL, edge=edge, lakes=lakes)
        torch.cuda.synchronize()
        return _keyed(rec, off), off.copy(), unc.copy()

    keyed, off, unc = _thrice(eng, device, tag + ("device",))
    _check_lists(_records(keyed), off, unc, want, tag + ("device",))
    # arrival: the planes of a finished segmenting transform on another context
    src = _engine(pkg, stream)
    simg, sseeds = _to_dev(torch, src, ref)
    labels = src.segment(simg, sseeds, max_level=MAXLVL, edge=edge)
    keys = src.last_arrival().clone()
    torch.cuda.synchronize()
    arr = _engine(pkg, stream)
    _live(pkg, arr, live)
    ph, pw = labels.shape
    opt = pkg._ffi.Options(MAXLVL, int(edge))
    cap = lakes.shape[0]

    def arrival():
        n = ctypes.c_size_t(0)
        o, u = np.zeros(LEVELS + 1, dtype=np.uint64), np.zeros(LEVELS, dtype=np.uint64)
        arr.ctx.check(pkg._ffi.lib().ws_lists_from_arrival_device(arr.ctx.handle, int(merging), keys.data_ptr(), labels.data_ptr(), ph, pw,
                                                                   len(ref["seeds"]), ctypes.byref(opt), lakes.data_ptr(), cap, ctypes.byref(n),
                                                                   o.ctypes.data, u.ctypes.data))
        torch.cuda.synchronize()
        return _keyed(lakes[: n.value], o), o, u

    keyed, off, unc = _thrice(arr, arrival, tag + ("arrival",))
    _check_lists(_records(keyed), off, unc, want, tag + ("arrival",))


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("merging,live", LIST_MODES)
def test_lists_stacked_batch(pkg, torch, stream, merging, live, edge):
    refs = _ref(edge)["stack"]
    eng = _engine(pkg, stream)
    _live(pkg, eng, live)
    cube, seeds, offs = _stack_to_dev(torch, eng, refs)
    lakes = torch.zeros((LEVELS * (offs[-1] + SLICES), 2), dtype=torch.int64, device=eng.device)

    def batch():
        rec, off, unc = eng.transform_to_list_batch(cube, seeds, offs, merging=merging, max_level=MAXLVL, edge=edge, lakes=lakes)
        torch.cuda.synchronize()
        assert len(off) == SLICES * LEVELS + 1 and int(off[-1]) == rec.shape[0]
        return _keyed(rec, off), off.copy(), unc.copy()

    keyed, off, unc = _thrice(eng, batch, ("batch lists", merging, live, edge), level_loop=not edge)
    for k, r in enumerate(refs):
        _check_lists(_records(keyed), off, unc, r["mer_sizes"] if merging else r["seg_sizes"], ("batch lists", merging, live, edge, k), first=k * LEVELS)


@pytest.mark.parametrize("edge", [False, True])
def test_hook_and_final_labels(pkg, torch, stream, edge):
    ref = _ref(edge)["field"]
    b = pkg.TransformBuilder.new().set_max_water_lvl(MAXLVL).set_context(pkg.api.Context(0))
    if edge:
        b.enable_edge_correction()
    ws = b.build_merging()
    hook = ws.transform_history(ref["img"], ref["seeds"])                # ws_merge_with_hook with a hook
    assert [l for l, _ in hook] == list(range(LEVELS))
    assert (np.stack([p for _, p in hook]) == ref["mer_planes"]).all()
    assert (ws.transform_final(ref["img"], ref["seeds"]) == ref["mer_planes"][MAXLVL]).all()      # ... and with none: final labels
    # final labels of a device image (ws_merge_device) and of the stacked batch (ws_merge_batch_device): no level loop
    eng = _engine(pkg, stream)
    img, seeds = _to_dev(torch, eng, ref)
    out = torch.zeros(ref["mer_planes"].shape[1:], dtype=torch.int32, device=eng.device)

    def device():
        eng.merge(img, seeds, max_level=MAXLVL, edge=edge, out=out)
        torch.cuda.synchronize()
        return (out.cpu().numpy().view(np.uint32),)

    got, = _thrice(eng, device, ("final labels", edge, "device"), level_loop=False)
    assert (got == ref["mer_planes"][MAXLVL]).all(), ("final labels", edge, "device")
    refs = _ref(edge)["stack"]
    bat = _engine(pkg, stream)
    cube, bseeds, offs = _stack_to_dev(torch, bat, refs)
    bout = torch.zeros((SLICES,) + refs[0]["mer_planes"].shape[1:], dtype=torch.int32, device=bat.device)

    def batch():
        bat.merge_batch(cube, bseeds, offs, max_level=MAXLVL, edge=edge, out=bout)
        torch.cuda.synchronize()
        return (bout.cpu().numpy().view(np.uint32),)

    got, = _thrice(bat, batch, ("final labels", edge, "batch"), level_loop=False)
    for k, r in enumerate(refs):
        assert (got[k] == r["mer_planes"][MAXLVL]).all(), ("final labels", edge, "batch", k)


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("merging", [False, True])
def test_history_host_device_batch(pkg, torch, stream, merging, edge):
    ref = _ref(edge)
    key = "mer_planes" if merging else "seg_planes"
    tag = ("history", merging, edge)
    b = pkg.TransformBuilder.new().set_max_water_lvl(MAXLVL).set_context(pkg.api.Context(0))
    if edge:
        b.enable_edge_correction()
    host = (b.build_merging() if merging else b.build_segmenting()).transform_history_levels(ref["field"]["img"], ref["field"]["seeds"])
    assert (np.stack([p for _, p in host]) == ref["field"][key]).all(), tag + ("host",)
    eng = _engine(pkg, stream)
    img, seeds = _to_dev(torch, eng, ref["field"])
    out = torch.zeros((LEVELS,) + ref["field"][key].shape[1:], dtype=torch.int32, device=eng.device)

    def device():
        eng.transform_history(img, seeds, merging=merging, max_level=MAXLVL, edge=edge, out=out)
        torch.cuda.synchronize()
        return (out.cpu().numpy().view(np.uint32),)

    got, = _thrice(eng, device, tag + ("device",), level_loop=merging)
    assert (got == ref["field"][key]).all(), tag + ("device",)
    bat = _engine(pkg, stream)
    cube, bseeds, offs = _stack_to_dev(torch, bat, ref["stack"])
    bout = torch.zeros((SLICES, LEVELS) + ref["stack"][0][key].shape[1:], dtype=torch.int32, device=bat.device)

    def batch():
        bat.transform_history_batch(cube, bseeds, offs, merging=merging, max_level=MAXLVL, edge=edge, out=bout)
        torch.cuda.synchronize()
        return (bout.cpu().numpy().view(np.uint32),)

    planes, = _thrice(bat, batch, tag + ("batch",), level_loop=merging and not edge)
    for k, r in enumerate(ref["stack"]):
        assert (planes[k] == r[key]).all(), tag + ("batch", k)


@pytest.mark.parametrize("edge", [False, True])
def test_tree_and_tree_with_statistics(pkg, torch, stream, edge):
    ref = _ref(edge)
    field = ref["field"]
    tag = ("tree", edge)
    b = pkg.TransformBuilder.new().set_max_water_lvl(MAXLVL).set_context(pkg.api.Context(0))
    if edge:
        b.enable_edge_correction()
    ws = b.build_merging()
    as_rows = lambda t: np.stack([t.parent, t.death_level, t.area, t.n_leaves], axis=1)
    # host: the tree (with labels), the tree with statistics
    t = ws.merge_tree(field["img"], field["seeds"], want_labels=True)
    assert (as_rows(t) == field["tree"]).all() and (t.labels == field["seg_planes"][MAXLVL]).all(), tag + ("host",)
    t, stats = ws.merge_tree_stats(field["img"], field["seeds"])
    assert (as_rows(t) == field["tree"]).all() and ls.mismatch(stats, field["stats"]) is None, tag + ("host stats", ls.mismatch(stats, field["stats"]))
    # device, each three times
    eng = _engine(pkg, stream)
    img, seeds = _to_dev(torch, eng, field)

    def tree():
        got, labels = eng.merge_tree(img, seeds, max_level=MAXLVL, edge=edge, want_labels=True)
        torch.cuda.synchronize()
        return got.cpu().numpy().view(np.uint32), labels.cpu().numpy().view(np.uint32)

    got, labels = _thrice(eng, tree, tag + ("device",))
    assert (got == field["tree"]).all() and (labels == field["seg_planes"][MAXLVL]).all(), tag + ("device",)
    eng2 = _engine(pkg, stream)
    img2, seeds2 = _to_dev(torch, eng2, field)

    def tree_stats():
        got, raw = eng2.merge_tree_stats(img2, seeds2, max_level=MAXLVL, edge=edge)
        torch.cuda.synchronize()
        return got.cpu().numpy().view(np.uint32), raw.cpu().numpy()

    got, raw = _thrice(eng2, tree_stats, tag + ("device stats",))
    assert (got == field["tree"]).all() and ls.mismatch(ls.from_raw(raw), field["stats"]) is None, tag + ("device stats",)
    # the stacked batch
    bat = _engine(pkg, stream)
    cube, bseeds, offs = _stack_to_dev(torch, bat, ref["stack"])

    def tree_batch():
        got, labels = bat.merge_tree_batch(cube, bseeds, offs, max_level=MAXLVL, edge=edge, want_labels=True)
        torch.cuda.synchronize()
        return got.cpu().numpy().view(np.uint32), labels.cpu().numpy().view(np.uint32)

    trees, labels = _thrice(bat, tree_batch, tag + ("batch",), level_loop=not edge)
    for k, r in enumerate(ref["stack"]):
        assert (trees[offs[k] + k: offs[k + 1] + k + 1] == r["tree"]).all(), tag + ("batch", k)
        assert (labels[k] == r["seg_planes"][MAXLVL]).all(), tag + ("batch labels", k)


@pytest.mark.parametrize("merging,live", LIST_MODES)
def test_lists_capacity_one_record_short(pkg, torch, stream, merging, live):
    ref = _ref(False)["field"]
    want = ref["mer_sizes"] if merging else ref["seg_sizes"]
    total = sum(int(np.count_nonzero(w[1:])) for w in want)
    eng = _engine(pkg, stream)
    _live(pkg, eng, live)
    img, seeds = _to_dev(torch, eng, ref)
    lakes = torch.zeros((total, 2), dtype=torch.int64, device=eng.device)
    n = ctypes.c_size_t(0)
    off, unc = np.zeros(LEVELS + 1, dtype=np.uint64), np.zeros(LEVELS, dtype=np.uint64)
    opt = eng.options(MAXLVL)

    def run(cap):
        return pkg._ffi.lib().ws_transform_to_list_device(eng.ctx.handle, int(merging), img.data_ptr(), H, W, W, seeds.data_ptr(), seeds.shape[0],
                                                          ctypes.byref(opt), lakes.data_ptr(), cap, ctypes.byref(n), off.ctypes.data, unc.ctypes.data)

    assert run(total - 1) == pkg._ffi.WS_ERR_CAPACITY and n.value == total
    assert run(total) == 0 and n.value == total
    torch.cuda.synchronize()
    _check_lists(lakes.cpu().numpy(), off, unc, want, ("capacity", merging, live))


def test_mode_switches_on_one_context_never_replay_the_other_graph(pkg, torch, stream):
    # lists, history, lists with the same shape on ONE context, each kind three times in a row so that its loop is captured and
    # replayed before the next kind takes over; then one call of each in turn
    ref = _ref(False)["field"]
    eng = _engine(pkg, stream)
    img, seeds = _to_dev(torch, eng, ref)
    lakes = torch.zeros((LEVELS * (len(ref["seeds"]) + 1), 2), dtype=torch.int64, device=eng.device)
    out = torch.zeros((LEVELS, H, W), dtype=torch.int32, device=eng.device)

    def lists():
        rec, off, unc = eng.transform_to_list(img, seeds, merging=True, max_level=MAXLVL, lakes=lakes)
        torch.cuda.synchronize()
        _check_lists(rec.cpu().numpy(), off, unc, ref["mer_sizes"], "switch lists")

    def history():
        out.zero_()
        eng.transform_history(img, seeds, merging=True, max_level=MAXLVL, out=out)
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == ref["mer_planes"]).all(), "switch history"

    for fn in (lists, history, lists):
        for _ in range(3):
            fn()
        assert eng.stats()["graph_launches"] > 0
    for fn in (history, lists, history, lists):
        fn()
