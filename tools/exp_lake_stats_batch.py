#!/usr/bin/env python3
"""ws_merge_tree_stats_batch(_device) (one stacked transform, one set of tree kernels and one set of statistics kernels for a cube)
against a loop of ws_merge_tree_stats(_device) over its slices on the same context, u16 weights: the device form with the records
in HBM both ways (equal records asserted), ws_merge_tree_batch_device alone (what the catalogue adds to the stacked tree), and the
host form (the C call with the seeds as one flat list, the Python wrapper) at 16 x 1024^2.  Median of K timed runs after warm-up,
a device synchronise around each.
usage: exp_lake_stats_batch.py [--out FILE.json] [--k K] [--config SxN:field] [--no-host] [--single-runs LABEL:FILE ...]
       exp_lake_stats_batch.py --one SxN      three batch calls at that size (the second captures the level loop, the third replays
                                              it), for rocprofv3 --kernel-trace --stats
--single-runs: results of tools/exp_lake_stats.py --sizes 1024 --route-max 0 written by alternate runs of the parent commit's
checkout and of this one (LABEL parent or branch), copied into the JSON as the evidence that the single-field call did not move."""
import argparse, ctypes, importlib, json, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge
pkg = ge.load_package()
import cases
dev = importlib.import_module("rustronomy_watershed_amd.device")

# (slices, plane side, field, host form too)
CONFIGS = [(16, 1024, "random", True), (8, 2048, "random", False), (16, 1024, "smooth", False)]

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lake_stats_batch.json"))
ap.add_argument("--k", type=int, default=7)
ap.add_argument("--config")
ap.add_argument("--one")
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--single-runs", nargs="*", default=[])
args = ap.parse_args()
if args.config:
    sn, kind = args.config.split(":")
    CONFIGS = [(int(sn.split("x")[0]), int(sn.split("x")[1]), kind, True)]
if args.one:
    CONFIGS = [(int(args.one.split("x")[0]), int(args.one.split("x")[1]), "random", False)]
torch.cuda.set_stream(torch.cuda.Stream(0))
eng = dev.DeviceEngine(0)


def timed(fn):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(args.k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


results = []
for s, n, kind, host in CONFIGS:
    if kind == "random":
        cube = torch.stack([eng.random_field(n, n, 1 + k) for k in range(s)]).contiguous()
    else:
        cube = torch.from_numpy(np.stack([cases.smooth_field(n, n, 1 + k) for k in range(s)])).to(eng.device).contiguous()
    hwt = np.stack([np.random.default_rng(100 + k).integers(0, 65536, (n, n), dtype=np.uint16) for k in range(s)])
    wt = torch.from_numpy(hwt.view(np.int16)).to(eng.device)
    lists = [eng.find_local_minima(cube[k]) for k in range(s)]
    offs = [0] + [int(x) for x in np.cumsum([int(l.shape[0]) for l in lists])]
    seeds = torch.cat(lists).contiguous()
    out = torch.empty((offs[-1] + s, 4), dtype=torch.int32, device=eng.device)
    raw = torch.empty((offs[-1] + s, 9), dtype=torch.int64, device=eng.device)
    outs = [out[offs[k] + k: offs[k + 1] + k + 1] for k in range(s)]
    raws = [raw[offs[k] + k: offs[k + 1] + k + 1] for k in range(s)]
    if args.one:
        for _ in range(3):
            eng.merge_tree_stats_batch(cube, seeds, offs, weights=wt, out=out, out_stats=raw)
        torch.cuda.synchronize()
        print(json.dumps({"one": args.one, "seeds": int(offs[-1]), "stats": {k: v for k, v in eng.stats().items() if "launch" in k}}))
        break
    batch_ms = timed(lambda: eng.merge_tree_stats_batch(cube, seeds, offs, weights=wt, out=out, out_stats=raw))
    st = eng.stats()
    got, got_raw = out.clone(), raw.clone()
    loop_ms = timed(lambda: [eng.merge_tree_stats(cube[k], lists[k], weights=wt[k], out=outs[k], out_stats=raws[k]) for k in range(s)])
    assert torch.equal(got, out) and torch.equal(got_raw, raw), "the batch and the loop disagree"
    tree_batch_ms = timed(lambda: eng.merge_tree_batch(cube, seeds, offs, out=out))
    assert torch.equal(got, out), "merge_tree_batch and the statistics batch disagree on the tree"
    r = {"slices": s, "plane": n, "field": kind, "weights": "u16", "seeds": int(offs[-1]), "batch_ms": batch_ms, "loop_ms": loop_ms,
         "speedup": loop_ms / batch_ms, "records_equal_loop": True, "tree_batch_ms": tree_batch_ms,
         "batch_minus_tree_batch_ms": batch_ms - tree_batch_ms, "batch_launches_relax": st["launches_relax"],
         "batch_graph_launches": st["graph_launches"]}
    if host and not args.no_host:
        ws = pkg.TransformBuilder.new().build_merging()
        hcube = cube.cpu().numpy()
        hseeds = [l.cpu().numpy().astype(np.uint64) for l in lists]
        flat = np.ascontiguousarray(np.concatenate(hseeds, axis=0))
        soffs = np.zeros(s + 1, dtype=np.uintp)
        soffs[1:] = np.cumsum([len(x) for x in hseeds])
        htree = np.empty((offs[-1] + s, 4), dtype=np.uint32)
        hstats = np.empty(offs[-1] + s, dtype=pkg.api.LAKE_STATS_DTYPE)
        ctx = ws._ctx()
        r["host_batch_ms"] = timed(lambda: ctx.check(pkg._ffi.lib().ws_merge_tree_stats_batch(
            ctx.handle, hcube.ctypes.data, s, n, n, n, n * n, flat.ctypes.data, soffs.ctypes.data_as(pkg._ffi.szp),
            ctypes.byref(ws._opt), hwt.ctypes.data, pkg._ffi.WS_DTYPES["uint16"], n, n * n, htree.ctypes.data, hstats.ctypes.data,
            htree.shape[0], None, None, None, None)))
        assert (htree.view(np.int32) == got.cpu().numpy()).all() and (hstats.view(np.int64).reshape(-1, 9) == got_raw.cpu().numpy()).all()
        r["host_wrapper_batch_ms"] = timed(lambda: ws.merge_tree_stats_cube(hcube, seeds=hseeds, weights=hwt))
        r["host_loop_ms"] = timed(lambda: [ws.merge_tree_stats(hcube[k], hseeds[k], weights=hwt[k]) for k in range(s)])
        r["host_speedup"] = r["host_loop_ms"] / r["host_batch_ms"]
        r["host_wrapper_speedup"] = r["host_loop_ms"] / r["host_wrapper_batch_ms"]
    results.append(r)
    print(json.dumps(r), flush=True)
    del out, outs, raw, raws
    torch.cuda.empty_cache()
if not args.one:
    res = {"tool": "tools/exp_lake_stats_batch.py", "k": args.k, "results": results}
    runs = []
    for item in args.single_runs:
        label, path = item.split(":", 1)
        with open(path) as f:
            runs.append({"checkout": label, "rows": [{k: r[k] for k in ("size", "stats_ms", "tree_ms")} for r in json.load(f)["rows"]]})
    if runs:
        res["single_field_parent_vs_branch"] = {"what": "tools/exp_lake_stats.py --sizes 1024 --route-max 0 of the parent commit's checkout and "
                                                        "of this one, run alternately in this order", "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
