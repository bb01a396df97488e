"""Times merge_tree (ws_merge_tree_device) against what it is built on and against today's route to the same hierarchy.

  python tools/exp_merge_tree.py [--sizes 1024 4096] [--out FILE]      all legs -> JSON (default: profiles/merge_tree.json) and,
                                                                       on stdout, the "Measured" bullet of DESIGN.md section 4.2
  python tools/exp_merge_tree.py --one 4096                            two device tree calls at that size, the first capturing the
                                                                       level loop, the second replaying it (for rocprofv3
                                                                       --kernel-trace --stats)

The bench's random field (ws_random_field_device), seeds from find_local_minima.  Legs, per size:
  tree_ms              (a) ws_merge_tree_device, records left in HBM
  history_1_level_ms   (b) ws_transform_history_device(merging) with ONE level: the same flood and stamped level loop plus one
                       plane, so (a) - (b) is about what the tree's own kernels cost
  tree_labels_ms       (a) with the segmenting labels copied out as well
  planes_route_ms      (c) today's route, up to --route-max only: all 255 merging history planes into HBM, then the host
                       derivation of the same records from them (planes_device_ms: the device part alone)
Wall-clock milliseconds, median of --reps (7), the first call of each leg not counted (graph capture, buffers)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, reps, sync):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def tree_from_planes(planes, seeds):
    """The records from the 255 canonical planes (numpy, host): the definition of ws_merge_tree, for distinct seed pixels.
    (tests/merge_tree_ref.py follows the definition colour by colour, duplicates included; this one is vectorised, so that the
    route's time is the planes and a fair derivation, not a Python loop over 10^5 colours.)"""
    S = seeds.shape[0]
    vals = planes[:, seeds[:, 0], seeds[:, 1]]                      # (levels, S): P_L at every seed pixel
    own = np.arange(1, S + 1, dtype=planes.dtype)
    gone = vals != own
    dies = gone.any(axis=0)
    death = np.where(dies, gone.argmax(axis=0), 0xFFFFFFFF).astype(np.uint32)
    parent = np.where(dies, vals[np.minimum(death, planes.shape[0] - 1).astype(np.int64), np.arange(S)], 0).astype(np.uint32)
    before = np.where(dies, death.astype(np.int64) - 1, planes.shape[0] - 1)
    area = np.ones(S, dtype=np.uint32)
    leaves = np.ones(S, dtype=np.uint32)
    for L in np.unique(before[before >= 0]):
        at = np.flatnonzero(before == L)
        area[at] = np.bincount(planes[L].ravel(), minlength=S + 1)[at + 1]
        leaves[at] = np.bincount(vals[L], minlength=S + 1)[at + 1]
    return parent, death, area, leaves


def design_bullet(rows):
    """The measured figures as the bullet DESIGN.md section 4.2 carries."""
    parts = []
    for r in rows:
        t = (f"{r['size']}² ({r['seeds'] / 1e6:.2f} M seeds): tree {r['tree_ms']} ms, one-level merging history {r['history_1_level_ms']} ms, "
             f"difference {r['tree_minus_history_ms']} ms")
        if "planes_route_ms" in r:
            t += f"; 255 planes into HBM {r['planes_device_ms']} ms, with the host derivation {r['planes_route_ms']} ms"
        parts.append(t)
    return "* **Measured** (`profiles/merge_tree.json`, `tools/exp_merge_tree.py`; wall ms, median of 7, one MI355X). " + ". ".join(parts) + "."


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--route-max", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_tree.json"))
    ap.add_argument("--one", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.load_package()
    dev = __import__("rustronomy_watershed_amd.device", fromlist=["DeviceEngine"])
    torch.cuda.set_stream(torch.cuda.Stream(0))
    eng = dev.DeviceEngine(0)
    sync = torch.cuda.synchronize
    if args.one:
        img = eng.random_field(args.one, args.one, 1)
        seeds = eng.find_local_minima(img)
        out = eng.merge_tree(img, seeds)
        sync()
        eng.merge_tree(img, seeds, out=out)
        sync()
        print(json.dumps({"one": args.one, "seeds": int(seeds.shape[0])}))
        return
    rows = []
    for size in args.sizes:
        img = eng.random_field(size, size, 1)
        seeds = eng.find_local_minima(img)
        ns = int(seeds.shape[0])
        row = {"field": "random", "size": size, "seeds": ns}
        out = torch.empty((ns + 1, 4), dtype=torch.int32, device=eng.device)
        row["tree_ms"] = _timed(lambda: eng.merge_tree(img, seeds, out=out), args.reps, sync)
        plane = torch.empty((1, size, size), dtype=torch.int32, device=eng.device)
        row["history_1_level_ms"] = _timed(lambda: eng.transform_history(img, seeds, levels=[254], merging=True, out=plane), args.reps, sync)
        row["tree_minus_history_ms"] = round(row["tree_ms"] - row["history_1_level_ms"], 3)
        row["tree_labels_ms"] = _timed(lambda: eng.merge_tree(img, seeds, out=out, want_labels=True), args.reps, sync)
        row["tree_bytes"] = (ns + 1) * 16
        if size <= args.route_max:
            planes = torch.empty((255, size, size), dtype=torch.int32, device=eng.device)
            row["planes_device_ms"] = _timed(lambda: eng.transform_history(img, seeds, merging=True, out=planes), args.reps, sync)
            hseeds = seeds.cpu().numpy().astype(np.int64)
            got = {}

            def route():
                eng.transform_history(img, seeds, merging=True, out=planes)
                got["tree"] = tree_from_planes(planes.cpu().numpy(), hseeds)
            row["planes_route_ms"] = _timed(route, max(1, args.reps // 3), sync)
            rec = eng.merge_tree(img, seeds, out=out).cpu().numpy().view(np.uint32)
            row["route_equals_tree"] = bool(all((rec[1:, k] == got["tree"][k]).all() for k in range(4)))
            del planes
        print(json.dumps(row), flush=True)
        rows.append(row)
    res = {"what": "merge_tree (ws_merge_tree_device) vs a one-level merging transform_history and vs the 255-plane route, wall ms "
                   "(median of 7), one MI355X; see tools/exp_merge_tree.py", "rows": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(design_bullet(rows))


if __name__ == "__main__":
    main()
