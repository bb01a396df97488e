#!/usr/bin/env python3
"""ws_merge_tree_batch(_device) (one stacked transform and one set of tree kernels for a cube) against a loop of
ws_merge_tree(_device) over its slices on the same context: the device form with the records in HBM both ways, and the host form
(the C call with the seeds as one flat list, the Python wrapper with per-slice lists, and the wrapper's minima form) at 16 x 1024^2.
Median of K timed runs after warm-up, a device synchronise around each.
usage: exp_merge_tree_batch.py [--out FILE.json] [--k K] [--config SxN:field] [--no-host]
       exp_merge_tree_batch.py --one SxN      three batch calls at that size (the second captures the level loop, the third replays
                                              it), for rocprofv3 --kernel-trace --stats"""
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
ap.add_argument("--out")
ap.add_argument("--k", type=int, default=7)
ap.add_argument("--config")
ap.add_argument("--one")
ap.add_argument("--no-host", action="store_true")
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
    lists = [eng.find_local_minima(cube[k]) for k in range(s)]
    offs = [0] + [int(x) for x in np.cumsum([int(l.shape[0]) for l in lists])]
    seeds = torch.cat(lists).contiguous()
    out = torch.empty((offs[-1] + s, 4), dtype=torch.int32, device=eng.device)
    outs = [out[offs[k] + k: offs[k + 1] + k + 1] for k in range(s)]
    if args.one:
        for _ in range(3):
            eng.merge_tree_batch(cube, seeds, offs, out=out)
        torch.cuda.synchronize()
        print(json.dumps({"one": args.one, "seeds": int(offs[-1]), "stats": {k: v for k, v in eng.stats().items() if "launch" in k}}))
        break
    batch_ms = timed(lambda: eng.merge_tree_batch(cube, seeds, offs, out=out))
    st = eng.stats()
    got = out.clone()
    loop_ms = timed(lambda: [eng.merge_tree(cube[k], lists[k], out=outs[k]) for k in range(s)])
    assert torch.equal(got, out), "the batch and the loop disagree"
    r = {"slices": s, "plane": n, "field": kind, "seeds": int(offs[-1]), "batch_ms": batch_ms, "loop_ms": loop_ms,
         "speedup": loop_ms / batch_ms, "batch_launches_relax": st["launches_relax"], "batch_graph_launches": st["graph_launches"]}
    if host and not args.no_host:
        ws = pkg.TransformBuilder.new().build_merging()
        hcube = cube.cpu().numpy()
        hseeds = [l.cpu().numpy().astype(np.uint64) for l in lists]
        flat = np.ascontiguousarray(np.concatenate(hseeds, axis=0))
        soffs = np.zeros(s + 1, dtype=np.uintp)
        soffs[1:] = np.cumsum([len(x) for x in hseeds])
        htree = np.empty((offs[-1] + s, 4), dtype=np.uint32)
        ctx = ws._ctx()
        r["host_batch_ms"] = timed(lambda: ctx.check(pkg._ffi.lib().ws_merge_tree_batch(
            ctx.handle, hcube.ctypes.data, s, n, n, n, n * n, flat.ctypes.data, soffs.ctypes.data_as(pkg._ffi.szp),
            ctypes.byref(ws._opt), htree.ctypes.data, htree.shape[0], None, None, None, None)))
        r["host_wrapper_batch_ms"] = timed(lambda: ws.merge_tree_cube(hcube, seeds=hseeds))
        r["host_wrapper_minima_batch_ms"] = timed(lambda: ws.merge_tree_cube(hcube))
        r["host_loop_ms"] = timed(lambda: [ws.merge_tree(hcube[k], hseeds[k]) for k in range(s)])
        r["host_speedup"] = r["host_loop_ms"] / r["host_batch_ms"]
        r["host_wrapper_speedup"] = r["host_loop_ms"] / r["host_wrapper_batch_ms"]
    results.append(r)
    print(json.dumps(r), flush=True)
    del out, outs
    torch.cuda.empty_cache()
if args.out and not args.one:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/exp_merge_tree_batch.py", "k": args.k, "results": results}, f, indent=1)
