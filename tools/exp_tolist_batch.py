#!/usr/bin/env python3
"""ws_transform_to_list_batch_device (one stacked transform for a cube) against a loop of ws_transform_to_list_device over its
slices, merging and segmenting, records in HBM both ways.  Median of K timed runs after warm-up, a device synchronise around each.
usage: exp_tolist_batch.py [--out FILE.json] [--once] [--k K] [--config SxN:field] [--leg batch|loop] [--merging-only]
  --once: every configuration once, untimed (the run to put under rocprofv3 --kernel-trace --stats); --config / --leg /
  --merging-only narrow it to one shape, one side, the merging transform"""
import argparse, importlib, json, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge
ge.load_package()
import cases
dev = importlib.import_module("rustronomy_watershed_amd.device")

CONFIGS = [(16, 1024, "random"), (64, 1024, "random"), (8, 2048, "random"), (16, 1024, "smooth")]

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--once", action="store_true")
ap.add_argument("--k", type=int, default=5)
ap.add_argument("--config")
ap.add_argument("--leg", choices=["batch", "loop"])
ap.add_argument("--merging-only", action="store_true")
args = ap.parse_args()
if args.config:
    sn, kind = args.config.split(":")
    CONFIGS = [(int(sn.split("x")[0]), int(sn.split("x")[1]), kind)]
torch.cuda.set_stream(torch.cuda.Stream(0))
eng = dev.DeviceEngine(0)


def timed(fn):
    if args.once:
        fn()
        return None
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
for s, n, kind in CONFIGS:
    if kind == "random":
        cube = torch.stack([eng.random_field(n, n, 1 + k) for k in range(s)]).contiguous()
    else:
        cube = torch.from_numpy(np.stack([cases.smooth_field(n, n, 1 + k) for k in range(s)])).to(eng.device).contiguous()
    lists = [eng.find_local_minima(cube[k]) for k in range(s)]
    offs = [0] + list(np.cumsum([int(l.shape[0]) for l in lists]))
    seeds = torch.cat(lists).contiguous()
    for merging in ((True,) if args.merging_only else (True, False)):
        # buffers sized by a first call of the side that is measured (under a trace, the other side never runs)
        if args.leg != "loop":
            lakes, off, _ = eng.transform_to_list_batch(cube, seeds, offs, merging=merging)
            per_slice = [int(off[(k + 1) * 255] - off[k * 255]) for k in range(s)]
        else:
            per_slice = [int(eng.transform_to_list(cube[k], lists[k], merging=merging)[1][-1]) for k in range(s)]
        lakes = None
        records = sum(per_slice)
        buf = torch.empty((records + 16, 2), dtype=torch.int64, device=eng.device) if args.leg != "loop" else None
        one_buf = torch.empty((max(per_slice) + 16, 2), dtype=torch.int64, device=eng.device)
        batch_ms = timed(lambda: eng.transform_to_list_batch(cube, seeds, offs, merging=merging, lakes=buf)) if args.leg != "loop" else None
        st = eng.stats()
        loop_ms = timed(lambda: [eng.transform_to_list(cube[k], lists[k], merging=merging, lakes=one_buf) for k in range(s)]) \
            if args.leg != "batch" else None
        r = {"slices": s, "plane": n, "field": kind, "merging": merging, "seeds": int(offs[-1]), "records": records,
             "batch_ms": batch_ms, "loop_ms": loop_ms, "speedup": (loop_ms / batch_ms) if batch_ms and loop_ms else None,
             "batch_launches_relax": st["launches_relax"], "batch_graph_launches": st["graph_launches"]}
        results.append(r)
        print(json.dumps(r), flush=True)
        del buf, one_buf
        torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/exp_tolist_batch.py", "k": args.k, "results": results}, f, indent=1)
