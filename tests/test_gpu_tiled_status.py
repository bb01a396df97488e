"""The argument checks of every tiled entry point (csrc/ws_tiled.hip), -m gpu: the six device forms and the four host forms on
local groups of 1, 2 and 4 ranks on device 0, one group per world for the module.  An 8 x 8 field with five seeds.

For each entry point: every call that is wrong in ONE way the code tells apart returns the status written here and leaves a
non-empty ws_group_last_error, and the same group then runs one good call of the same entry point whose result equals the
single-context call's on the whole field, bit for bit.  Calls wrong in two ways are not asserted (include/ws_hip.h names the order
of the checks).  Every refused call returns before any work is queued: nothing here reaches a kernel with a bad argument."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

H = W = 8
SEEDS = np.array([[0, 2], [2, 6], [3, 3], [5, 1], [7, 4]], dtype=np.int64)      # row-major increasing: contiguous ranges per row block
N = len(SEEDS)
GRID = {1: (1, 1), 2: (1, 2), 4: (2, 2)}
IMG = np.random.default_rng(88).integers(0, 256, (H, W), dtype=np.uint8)
WEIGHT = np.random.default_rng(89).integers(0, 65536, (H, W), dtype=np.uint16)
TOO_MANY = (1 << 31) - 1
CAP = N * 255 + 16


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
    grp_mod = importlib.import_module("rustronomy_watershed_amd.group")
    gs = {world: grp_mod.Group.local(world) for world in (1, 2, 4)}
    yield gs
    for g in gs.values():
        g.close()


@pytest.fixture(scope="module")
def want(pkg, eng):
    """The single-context results, once: labels, (records, offsets, uncoloured) of the merging lists, (tree, catalogue)."""
    import torch
    t_img = torch.from_numpy(IMG).to(eng.device)
    t_seeds = torch.from_numpy(SEEDS.astype(np.int32)).to(eng.device)
    t_wt = torch.from_numpy(WEIGHT.view(np.int16)).to(eng.device)
    labels = eng.segment(t_img, t_seeds)
    lakes, offsets, unc = eng.transform_to_list(t_img, t_seeds, merging=True)
    tree, stats = eng.merge_tree_stats(t_img, t_seeds, weights=t_wt)
    torch.cuda.synchronize()
    return {"t_img": t_img, "t_seeds": t_seeds, "t_wt": t_wt, "labels": labels.cpu().numpy().view(np.uint32),
            "lakes": lakes.cpu().numpy().view(np.uint64).copy(), "offsets": offsets.copy(), "unc": unc.copy(),
            "tree": tree.cpu().numpy().view(np.uint32).copy(), "stats": stats.cpu().numpy().copy()}


def _copy_blocks(blocks, edit):
    """A copy of the descriptor array with `edit` applied to the LAST local block (every loop over the blocks must reach it)."""
    out = type(blocks)()
    for i in range(len(blocks)):
        out[i] = type(blocks[i]).from_buffer_copy(blocks[i])
    for k, v in edit.items():
        setattr(out[len(blocks) - 1], k, v)
    return out


class Calls:
    """The ten entry points on one group: call(name, **wrong) runs the good call with the named arguments replaced."""

    def __init__(self, pkg, eng, g, want):
        import torch
        self.torch, self.ffi, self.L, self.g, self.want = torch, pkg._ffi, pkg._ffi.lib(), g, want
        self.world = g.world
        self.py, self.px = GRID[g.world]
        t_img, t_seeds = want["t_img"], want["t_seeds"]
        self.rows, self.row_spans, self.keep1 = g.make_blocks(H, lambda lo, hi, rank: t_img[lo:hi].contiguous(), t_seeds)
        self.tiles, self.tile_spans, self.keep2 = g.make_blocks2d(t_img, t_seeds, self.py, self.px)
        self.d_lakes = torch.zeros((CAP, 2), dtype=torch.int64, device=eng.device)
        self.d_tree = torch.zeros((N + 1, 4), dtype=torch.int32, device=eng.device)
        self.d_stats = torch.zeros((N + 1, 9), dtype=torch.int64, device=eng.device)
        self.seeds64 = np.ascontiguousarray(SEEDS.astype(np.uint64))
        self.out = np.zeros((H, W), dtype=np.uint64)
        self.lakes = np.zeros((CAP, 2), dtype=np.uint64)
        self.tree = np.zeros((N + 1, 4), dtype=np.uint32)
        self.stats = np.zeros((N + 1, 9), dtype=np.int64)
        self.n_lakes = ctypes.c_size_t(0)
        self.offsets, self.unc = np.zeros(256, dtype=np.uint64), np.zeros(255, dtype=np.uint64)
        self.u16 = self.ffi.WS_DTYPES["uint16"]

    # ---- arguments ------------------------------------------------------------------------------------------------------------------
    def _dev_args(self, two_d, wrong):
        a = {"blocks": self.tiles if two_d else self.rows, "opt": self.ffi.Options(254), "field_h": H, "field_w": W, "n_total": N,
             "py": self.py, "px": self.px, "d_lakes": self.d_lakes.data_ptr(), "cap": CAP, "n_lakes": ctypes.byref(self.n_lakes),
             "offsets": self.offsets.ctypes.data, "unc": self.unc.ctypes.data, "d_tree": self.d_tree.data_ptr(),
             "d_stats": self.d_stats.data_ptr(), "weight": self.want["t_wt"].data_ptr(), "dtype": self.u16, "wstride": W}
        block = wrong.pop("block", None)
        a.update(wrong)
        if block is not None:
            a["blocks"] = _copy_blocks(a["blocks"], block)
        a["opt"] = ctypes.byref(a["opt"]) if a["opt"] is not None else None
        return a

    def _host_args(self, wrong):
        a = {"img": IMG.ctypes.data, "h": H, "w": W, "stride": W, "seeds": self.seeds64.ctypes.data, "n": N, "opt": self.ffi.Options(254),
             "py": self.py, "px": self.px, "out": self.out.ctypes.data, "lakes": self.lakes.ctypes.data, "cap": CAP,
             "n_lakes": ctypes.byref(self.n_lakes), "offsets": self.offsets.ctypes.data, "unc": self.unc.ctypes.data,
             "tree": self.tree.ctypes.data, "stats": self.stats.ctypes.data, "weight": WEIGHT.ctypes.data, "dtype": self.u16, "wstride": W}
        if "seed_list" in wrong:
            self.bad_seeds = np.ascontiguousarray(np.asarray(wrong.pop("seed_list"), dtype=np.uint64).reshape(-1, 2))
            a["seeds"], a["n"] = (self.bad_seeds.ctypes.data if len(self.bad_seeds) else None), len(self.bad_seeds)
        a.update(wrong)
        a["opt"] = ctypes.byref(a["opt"]) if a["opt"] is not None else None
        return a

    # ---- the entry points -----------------------------------------------------------------------------------------------------------
    def call(self, name, **wrong):
        L, h = self.L, self.g._h
        if name.endswith("_device"):
            a = self._dev_args("2d" in name, wrong)
            grid = (a["field_h"], a["field_w"], a["py"], a["px"]) if "2d" in name else (a["field_h"], a["field_w"])
            lists = (a["d_lakes"], a["cap"], a["n_lakes"], a["offsets"], a["unc"], None)
            tree = (a["weight"], a["dtype"], a["wstride"], a["d_tree"], a["d_stats"], None)
            if name.startswith("ws_segment"):
                return getattr(L, name)(h, *grid, a["n_total"], a["blocks"], a["opt"], 0, None)
            if name.startswith("ws_transform_to_list"):
                return getattr(L, name)(h, *grid, a["n_total"], a["blocks"], a["opt"], 1, *lists)
            return getattr(L, name)(h, *grid, a["n_total"], a["blocks"], a["opt"], *tree)
        a = self._host_args(wrong)
        field = (a["img"], a["h"], a["w"], a["stride"], a["seeds"], a["n"], a["opt"])
        if name == "ws_segment_tiled":
            return L.ws_segment_tiled(h, *field, 0, a["out"], None)
        if name == "ws_segment_tiled2d":
            return L.ws_segment_tiled2d(h, *field, a["py"], a["px"], 0, a["out"], None)
        if name == "ws_transform_to_list_tiled":
            return L.ws_transform_to_list_tiled(h, 1, *field, a["lakes"], a["cap"], a["n_lakes"], a["offsets"], a["unc"], None)
        return L.ws_merge_tree_tiled(h, *field, a["weight"], a["dtype"], a["wstride"], a["tree"], a["stats"], None)

    def refused(self, name, what, status, wrong, message=None):
        rc = self.call(name, **dict(wrong))
        err = self.L.ws_group_last_error(self.g._h)
        assert rc == status, (name, self.world, what, rc, err)
        assert err, (name, self.world, what)
        if message is not None:
            assert message in err, (name, self.world, what, err)

    # ---- a good call equals the single-context result ---------------------------------------------------------------------------------
    def good(self, name, after):
        torch, want, tag = self.torch, self.want, (name, self.world, "after", after)
        device = name.endswith("_device")
        for _, _, _, lab in self.row_spans:
            lab.fill_(-1)
        for _, _, lab in self.tile_spans:
            lab.fill_(-1)
        for t in (self.d_lakes, self.d_tree, self.d_stats):
            t.fill_(77)
        for a in (self.out, self.lakes, self.tree, self.stats):
            a[...] = 77
        self.n_lakes.value = 0
        torch.cuda.synchronize()
        rc = self.call(name)
        assert rc == 0, (tag, rc, self.L.ws_group_last_error(self.g._h))
        torch.cuda.synchronize()
        if name == "ws_segment_tiled_device":
            for r0, r1, lo, lab in self.row_spans:
                assert (lab[r0 - lo:r1 - lo].cpu().numpy().view(np.uint32) == want["labels"][r0:r1]).all(), tag
        elif name == "ws_segment_tiled2d_device":
            for (r0, r1, lo, hi), (c0, c1, clo, chi), lab in self.tile_spans:
                assert (lab[r0 - lo:r1 - lo, c0 - clo:c1 - clo].cpu().numpy().view(np.uint32) == want["labels"][r0:r1, c0:c1]).all(), tag
        elif name in ("ws_segment_tiled", "ws_segment_tiled2d"):
            assert (self.out == want["labels"]).all(), tag
        elif name.startswith("ws_transform_to_list"):
            rec = self.d_lakes.cpu().numpy().view(np.uint64) if device else self.lakes
            n = len(want["lakes"])
            assert self.n_lakes.value == n and (rec[:n] == want["lakes"]).all(), tag
            assert (self.offsets == want["offsets"]).all() and (self.unc == want["unc"]).all(), tag
        else:
            tree = self.d_tree.cpu().numpy().view(np.uint32) if device else self.tree
            stats = self.d_stats.cpu().numpy() if device else self.stats
            assert (tree == want["tree"]).all() and (stats == want["stats"]).all(), tag


def mistakes(c, name):
    """(what, status, the arguments that make the call wrong in that one way[, a word the message must hold])."""
    ffi, world = c.ffi, c.world
    BAD, UNS, BIG = ffi.WS_ERR_BAD_ARG, ffi.WS_ERR_UNSUPPORTED, ffi.WS_ERR_TOO_LARGE
    dev, two_d = name.endswith("_device"), "2d" in name
    some_ptr = c.want["t_seeds"].data_ptr()      # a valid device pointer where a descriptor needs one beside the wrong field
    m = [("max_water_level 0", ffi.WS_ERR_MAX_TOO_LOW, {"opt": ffi.Options(0)}),
         ("null options", BAD, {"opt": None})]
    if world > 1:
        m.append(("the sweep engine", UNS, {"opt": ffi.Options(254, 0, ffi.WS_ENGINE_SWEEP)}))
    if two_d:
        m.append(("py * px is not the world", BAD, {"py": 2, "px": 3}))
    if dev:
        m += [("null blocks", BAD, {"blocks": None}),
              ("edge correction", UNS, {"opt": ffi.Options(254, 1)}),
              ("n_seeds_total 2^31 - 1", BIG, {"n_total": TOO_MANY}),
              ("null image", BAD, {"block": {"d_img": None}}),
              ("null labels", BAD, {"block": {"d_labels": None}}),
              ("seeds counted but not given", BAD, {"block": {"d_seeds_rc": None, "n_seeds": 1, "d_colours": some_ptr if two_d else None}})]
        if two_d:
            width = c.tile_spans[-1][1][3] - c.tile_spans[-1][1][2]
            m += [("fewer rows than tile rows", BAD, {"field_h": c.py - 1}),
                  ("fewer columns than tile columns", BAD, {"field_w": c.px - 1}),
                  ("img_stride below the tile's width", BAD, {"block": {"img_stride": width - 1}}),
                  ("seeds without colours", BAD, {"block": {"d_seeds_rc": some_ptr, "n_seeds": 1, "d_colours": None}})]
        else:
            m += [("fewer rows than ranks", BAD, {"field_h": world - 1}),
                  ("reserved is not 0", BAD, {"block": {"reserved": 1}})]
            if world == 1:
                m.append(("colours in a group of one", UNS, {"block": {"d_colours": some_ptr}}))
        if "to_list" in name:
            m += [("null n_lakes", BAD, {"n_lakes": None}), ("null offsets", BAD, {"offsets": None}), ("null uncoloured", BAD, {"unc": None}),
                  ("null d_lakes with a capacity", BAD, {"d_lakes": None})]
        if "merge_tree" in name:
            m += [("null d_tree", BAD, {"d_tree": None}),
                  ("the catalogue without weights", BAD, {"weight": None}, b"d_weight"),
                  ("weights of a wrong dtype", UNS, {"dtype": ffi.WS_DTYPES["float32"]}),
                  ("weight stride below w", BAD, {"wstride": W - 1})]
        return m
    m += [("null image", BAD, {"img": None}),
          ("seeds counted but not given", BAD, {"seeds": None}),
          ("img_stride below the width", BAD, {"stride": W - 1}),
          ("n_seeds 2^31 - 1", BIG, {"n": TOO_MANY}),
          ("a seed below the plane", ffi.WS_ERR_SEED_OOB, {"seed_list": [[0, 2], [H, 1]]}),
          ("a seed right of the plane", ffi.WS_ERR_SEED_OOB, {"seed_list": [[0, 2], [1, W]]})]
    if two_d:
        m += [("fewer rows than tile rows", BAD, {"h": c.py - 1, "seed_list": []}),
              ("fewer columns than tile columns", BAD, {"w": c.px - 1, "stride": W, "seed_list": []})]
    else:
        m.append(("fewer rows than ranks", BAD, {"h": world - 1, "seed_list": []}))
    if name.startswith("ws_segment"):
        m.append(("null out_labels", BAD, {"out": None}))
    if "to_list" in name:
        m += [("null n_lakes", BAD, {"n_lakes": None}), ("null offsets", BAD, {"offsets": None}), ("null uncoloured", BAD, {"unc": None}),
              ("null lakes with a capacity", BAD, {"lakes": None})]
    if "merge_tree" in name:
        m += [("null tree", BAD, {"tree": None}),
              ("weights of a wrong dtype", UNS, {"dtype": ffi.WS_DTYPES["float32"]}),
              ("weight stride below w", BAD, {"wstride": W - 1})]
    return m


ENTRY_POINTS = ["ws_segment_tiled_device", "ws_transform_to_list_tiled_device", "ws_merge_tree_tiled_device",
                "ws_segment_tiled2d_device", "ws_transform_to_list_tiled2d_device", "ws_merge_tree_tiled2d_device",
                "ws_segment_tiled", "ws_transform_to_list_tiled", "ws_merge_tree_tiled", "ws_segment_tiled2d"]

_CALLS = {}


@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_every_single_mistake_is_refused_and_a_good_call_follows(pkg, eng, groups, want, name, world):
    if world not in _CALLS:
        _CALLS[world] = Calls(pkg, eng, groups[world], want)
    c = _CALLS[world]
    c.good(name, "nothing")
    table = mistakes(c, name)
    assert len({t[0] for t in table}) == len(table)
    for what, status, wrong, *message in table:
        c.refused(name, what, status, wrong, *message)
        c.good(name, what)
