"""The final merged labels of ws_merge_device (union_image in csrc/ws_merge_final.hip: the one-lake tile route) on the duplicate seed
lists and the long tile runs of tests/final_merge_cases.py, -m gpu.  Every comparison is on all pixels, bit for bit, against the
CPU oracle (ol.merge_arrival); tests/test_final_merge_cases_cpu.py proves that the inputs are in their regimes.

The contract is the oracle's, and what every other entry point returns: a lake's id is the smallest colour in it that EXISTS --
whose seed pixel still carries it after seeding, where a later list entry on the same pixel overwrites an earlier one
(lib.rs:1670-1677).
"""
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import final_merge_cases as fm
import oracle_lib as ol
import strided

pytestmark = pytest.mark.gpu

D = fm.d_cases()
L = fm.l_cases()


def _ids(cs):
    return [c[0] for c in cs]


@pytest.fixture(scope="module")
def pkg():
    ge.build_hip()
    return ge.load_package()


@pytest.fixture(scope="module")
def dev(pkg):
    return importlib.import_module("rustronomy_watershed_amd.device")


# ---- the oracle, once per case ------------------------------------------------------------------------------------------------------

_WANT = {}


def _oracle(key, img, plane_seeds, facts):
    if key not in _WANT:
        v = ol.merge_arrival(img, plane_seeds, max_level=facts["max_level"], edge=facts["edge"])
        v.setflags(write=False)
        _WANT[key] = v
    return _WANT[key]


def want_of(case):
    return _oracle(case[0], case[1], fm.plane_seeds(case), case[3])


def _opts(facts):
    return {"max_level": facts["max_level"], "edge": facts["edge"], "seed_shift": facts["shift"]}


def _to_dev(eng, img, seeds):
    import torch
    t_img = torch.from_numpy(np.ascontiguousarray(img)).to(eng.device)
    t_seeds = torch.from_numpy(np.asarray(seeds, dtype=np.int64).reshape(-1, 2).astype(np.int32)).to(eng.device).contiguous()
    return t_img, t_seeds


def _np32(t):
    return t.cpu().numpy().view(np.uint32)


def _same(got, want, tag):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:3].tolist(), got[bad][:3].tolist(), want[bad][:3].tolist())


# ---- ws_merge_device against the oracle, every case, twice on one context ------------------------------------------------------------

def _merge_twice(dev, case):
    name, img, seeds, facts = case
    eng = dev.DeviceEngine(0)
    t_img, t_seeds = _to_dev(eng, img, seeds)
    want = want_of(case)
    for rep in range(2):
        _same(_np32(eng.merge(t_img, t_seeds, **_opts(facts))), want, (name, rep))


@pytest.mark.parametrize("case", D, ids=_ids(D))
def test_merge_device_on_duplicate_seed_lists(dev, case):
    _merge_twice(dev, case)


@pytest.mark.parametrize("case", L, ids=_ids(L))
def test_merge_device_on_long_runs_of_one_lake_tiles(dev, case):
    _merge_twice(dev, case)


# ---- the same lake, the same id, whichever entry point is asked ----------------------------------------------------------------------

@pytest.mark.parametrize("case", D, ids=_ids(D))
def test_entry_points_agree_on_duplicate_seed_lists(pkg, dev, case):
    import torch
    name, img, seeds, facts = case
    lvl = facts["max_level"]
    want = want_of(case)
    eng = dev.DeviceEngine(0)
    t_img, t_seeds = _to_dev(eng, img, seeds)
    merged = _np32(eng.merge(t_img, t_seeds, **_opts(facts)))
    _same(merged, want, (name, "ws_merge_device"))
    # the last plane of the merging history (no seed_shift there: the list goes in plane coordinates)
    _, t_plane_seeds = _to_dev(eng, img, fm.plane_seeds(case))
    hist = _np32(eng.transform_history(t_img, t_plane_seeds, levels=[lvl], merging=True, max_level=lvl, edge=facts["edge"]))
    _same(hist[0], merged, (name, "history"))
    # the host transform_final (merge_host)
    ctx = pkg.api.Context(0)
    try:
        b = pkg.TransformBuilder.new().set_context(ctx).set_max_water_lvl(lvl)
        if facts["edge"]:
            b = b.enable_edge_correction().shift_seeds_into_padded_plane(facts["shift"])
        final = b.build_merging().transform_final(img, np.ascontiguousarray(seeds.astype(np.uint64)))
    finally:
        ctx.close()
    _same(final.astype(np.uint32), merged, (name, "transform_final"))
    assert final.dtype == np.uint64 and (final == want).all()
    # the tree: roots_at(max) over its segmenting labels
    tree, labels = eng.merge_tree(t_img, t_seeds, want_labels=True, **_opts(facts))
    torch.cuda.synchronize()
    rec = _np32(tree)
    t = pkg.api.MergeTree(rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3])
    _same(t.roots_at(lvl)[_np32(labels)], merged, (name, "MergeTree.roots_at"))


def _groups():
    """D cases of one plane and one set of options, two or three to a cube; every D case is in exactly one."""
    by = {}
    for c in D:
        by.setdefault((c[1].shape, c[3]["edge"], c[3]["shift"], c[3]["max_level"]), []).append(c)
    out = []
    for key, cs in by.items():
        assert len(cs) >= 2, key
        k = 0
        while k < len(cs):
            left = len(cs) - k
            take = 2 if left in (2, 4) else 3
            out.append(cs[k:k + take])
            k += take
    return out


GROUPS = _groups()


@pytest.mark.parametrize("group", GROUPS, ids=[g[0][0] + f"+{len(g) - 1}" for g in GROUPS])
def test_merge_batch_slices_equal_single_calls_on_duplicate_seed_lists(dev, group):
    import torch
    assert 2 <= len(group) <= 3
    facts = group[0][3]
    eng = dev.DeviceEngine(0)
    lists = [c[2] for c in group]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    cube = torch.from_numpy(np.stack([c[1] for c in group])).to(eng.device)
    allseeds = torch.from_numpy(np.concatenate(lists).astype(np.int32)).to(eng.device).contiguous()
    got = _np32(eng.merge_batch(cube, allseeds, offs, **_opts(facts)))
    for k, case in enumerate(group):
        _same(got[k], want_of(case), (case[0], "batch slice", k))
        t_img, t_seeds = _to_dev(eng, case[1], case[2])
        _same(got[k], _np32(eng.merge(t_img, t_seeds, **_opts(facts))), (case[0], "batch against the single call", k))


# ---- replay: one context on a stream of its own, one set of device buffers -----------------------------------------------------------

def _replay_lists(h, w):
    """A strictly increasing list and three of the same count with other entries doubled: the last entry names the pixel of entry
    0 (colour 1 overwritten: the lake's id is 2), of entry 3, and entries 0 .. 2 again."""
    rng = np.random.default_rng(97)
    px = np.sort(rng.choice((h - 2) * (w - 2), size=40, replace=False))
    strict = np.stack([px // (w - 2) + 1, px % (w - 2) + 1], axis=1).astype(np.int64)
    a, b, c = strict.copy(), strict.copy(), strict.copy()
    a[-1] = strict[0]
    b[-1] = strict[3]
    b[10] = strict[3]
    c[-3:] = strict[:3]
    return strict, a, b, c


@pytest.mark.parametrize("kind", ["flat", "noise"])
def test_replayed_merge_with_the_seed_buffer_rewritten_in_place(dev, kind):
    import torch
    h, w = 72, 136      # W % 4 == 0: a strictly increasing list takes the seed tables, and only those transforms are captured
    img = fm.image(kind, h, w, np.random.default_rng(5))
    strict, a, b, c = _replay_lists(h, w)
    facts = {"max_level": 254, "edge": False}
    with torch.cuda.stream(torch.cuda.Stream()):      # capture is not allowed on the legacy null stream
        eng = dev.DeviceEngine(0)
        d_img = torch.from_numpy(img).to(eng.device)
        d_seeds = torch.empty((len(strict), 2), dtype=torch.int32, device=eng.device)
        out = torch.empty((h, w), dtype=torch.int32, device=eng.device)

        def put(lst):
            d_seeds.copy_(torch.from_numpy(lst).to(torch.int32))
            return _oracle((kind, "replay", lst.tobytes()), img, lst, facts)

        def whole():
            return _np32(eng.merge(d_img, d_seeds, out=out))

        def halves():
            eng.merge_begin(d_img, d_seeds, out)
            return _np32(eng.merge_end())

        for run, tag in ((whole, "merge"), (halves, "merge_begin / merge_end")):
            want = put(strict)
            for rep in range(4):
                _same(run(), want, (tag, "strict", rep))
            assert eng.stats()["graph_launches"] == 1, tag      # (as test_graph_replay_of_repeated_transforms)
            # the same buffers and count, the contents rewritten: the graph is replayed, its tables refuse the list, the unions
            # queued behind it ran on the previous labels and are done again
            for k, lst in enumerate((a, b, c, strict, a, strict, strict)):
                want = put(lst)
                _same(run(), want, (tag, "rewritten", k))
            assert not (_oracle((kind, "replay", a.tobytes()), img, a, facts) == 1).any()      # colour 1 is gone from list a


# ---- label plane forms: W % 4 != 0 (the scalar branch of k_tile_scan, the gather of k_relabel_tiles) and an `out` 4 bytes off ----------
# ---- 16-byte alignment (the gather on a plane whose width would allow the fill)

FORMS = [fm.named("D/72x136/then_reversed/noise/one"), fm.named("D/67x131/first_again/noise/one"), fm.named("L/832x320/"), fm.named("L/194x323/")]


@pytest.mark.parametrize("case", FORMS, ids=_ids(FORMS))
def test_merge_device_label_plane_forms(dev, case):
    import torch
    name, img, seeds, facts = case
    h, w = img.shape
    want = want_of(case)
    assert {c[1].shape[1] % 4 != 0 for c in FORMS} == {True, False}
    eng = dev.DeviceEngine(0)
    _, t_seeds = _to_dev(eng, img, seeds)
    guard = 64
    for img_off, out_off in ((0, 0), (0, 1), (1, 1), (3, 3)):
        # the image at a byte offset inside a larger allocation, random bytes around it
        backing, off, _ = strided.embed(img, img_off, w, ("random", 11))
        assert strided.GUARD % 16 == 0
        d_back = torch.from_numpy(backing).to(eng.device)
        t_img = d_back[off:off + h * w].view(h, w)
        assert t_img.is_contiguous() and t_img.data_ptr() % 16 == (d_back.data_ptr() + off) % 16
        buf = torch.full((guard + out_off + h * w + guard,), -1515870811, dtype=torch.int32, device=eng.device)      # 0xA5A5A5A5
        out = buf[guard + out_off:guard + out_off + h * w].view(h, w)
        assert out.data_ptr() % 16 == (4 * out_off) % 16
        for rep in range(2):
            got = _np32(eng.merge(t_img, t_seeds, out=out, **_opts(facts)))
            _same(got, want, (name, img_off, out_off, rep))
        whole = buf.cpu().numpy()
        assert (whole[:guard + out_off] == -1515870811).all() and (whole[guard + out_off + h * w:] == -1515870811).all(), (name, out_off)
