#!/usr/bin/env python3
"""ws_transform_history_batch(_device) (one stacked transform for a cube) against a loop of ws_transform_history(_device) over its
slices, merging and segmenting: the device form with the planes in HBM both ways, and the host form into a reused u64 array both
ways (the C call, the Python wrapper with per-slice seed lists -- it concatenates them -- and the wrapper's minima form).
Median of K timed runs after warm-up, a device synchronise around each.
usage: exp_history_batch.py [--out FILE.json] [--k K] [--config SxN:field:levels] [--no-host]"""
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

# (slices, plane side, field, number of levels, host form too): 32 levels of 16 x 1024^2 are 4 GiB of u64 on the host -- device only
CONFIGS = [(16, 1024, "random", 8, True), (16, 1024, "random", 32, False), (8, 2048, "random", 8, True), (16, 1024, "smooth", 8, True)]

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--k", type=int, default=5)
ap.add_argument("--config")
ap.add_argument("--no-host", action="store_true")
args = ap.parse_args()
if args.config:
    sn, kind, nl = args.config.split(":")
    CONFIGS = [(int(sn.split("x")[0]), int(sn.split("x")[1]), kind, int(nl), True)]
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
for s, n, kind, nl, host in CONFIGS:
    if kind == "random":
        cube = torch.stack([eng.random_field(n, n, 1 + k) for k in range(s)]).contiguous()
    else:
        cube = torch.from_numpy(np.stack([cases.smooth_field(n, n, 1 + k) for k in range(s)])).to(eng.device).contiguous()
    lists = [eng.find_local_minima(cube[k]) for k in range(s)]
    offs = [0] + [int(x) for x in np.cumsum([int(l.shape[0]) for l in lists])]
    seeds = torch.cat(lists).contiguous()
    levels = [int(x) for x in np.linspace(0, 254, nl).round()]
    out = torch.empty((s, nl, n, n), dtype=torch.int32, device=eng.device)
    for merging in (True, False):
        batch_ms = timed(lambda: eng.transform_history_batch(cube, seeds, offs, levels=levels, merging=merging, out=out))
        st = eng.stats()
        loop_ms = timed(lambda: [eng.transform_history(cube[k], lists[k], levels=levels, merging=merging, out=out[k]) for k in range(s)])
        r = {"slices": s, "plane": n, "field": kind, "levels": nl, "merging": merging, "seeds": int(offs[-1]),
             "batch_ms": batch_ms, "loop_ms": loop_ms, "speedup": loop_ms / batch_ms,
             "batch_launches_relax": st["launches_relax"], "batch_graph_launches": st["graph_launches"]}
        if host and not args.no_host:
            b = pkg.TransformBuilder.new()
            ws = b.build_merging() if merging else b.build_segmenting()
            hcube = cube.cpu().numpy()
            hseeds = [l.cpu().numpy().astype(np.uint64) for l in lists]
            hout = np.empty((s, nl, n, n), dtype=np.uint64)
            # the C call with the cube's seeds as one flat list (as the loop gets its slices' lists: ready), then the Python
            # wrapper, which concatenates the per-slice lists first, and its minima form (no lists at all)
            flat = np.ascontiguousarray(np.concatenate(hseeds, axis=0))
            soffs = np.zeros(s + 1, dtype=np.uintp)
            soffs[1:] = np.cumsum([len(x) for x in hseeds])
            lv = np.asarray(levels, dtype=np.uint8)
            ctx = ws._ctx()
            r["host_batch_ms"] = timed(lambda: ctx.check(pkg._ffi.lib().ws_transform_history_batch(
                ctx.handle, int(merging), hcube.ctypes.data, s, n, n, n, n * n, flat.ctypes.data, soffs.ctypes.data_as(pkg._ffi.szp),
                ctypes.byref(ws._opt), lv.ctypes.data, nl, hout.ctypes.data, None, None)))
            r["host_wrapper_batch_ms"] = timed(lambda: ws.transform_history_cube(hcube, seeds=hseeds, levels=levels, out=hout))
            r["host_wrapper_minima_batch_ms"] = timed(lambda: ws.transform_history_cube(hcube, levels=levels, out=hout))
            r["host_loop_ms"] = timed(lambda: [ws.transform_history_levels(hcube[k], hseeds[k], levels, out=hout[k]) for k in range(s)])
            r["host_speedup"] = r["host_loop_ms"] / r["host_batch_ms"]
            r["host_wrapper_speedup"] = r["host_loop_ms"] / r["host_wrapper_batch_ms"]
            del hout
        results.append(r)
        print(json.dumps(r), flush=True)
    del out
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/exp_history_batch.py", "k": args.k, "results": results}, f, indent=1)
