"""Times merge_tree_stats (ws_merge_tree_stats_device) against merge_tree and against today's route to the same catalogue.

  python tools/exp_lake_stats.py [--sizes 1024 4096] [--out FILE] [--tree-runs LABEL:FILE ...]
        all legs -> JSON (default: profiles/lake_stats.json) and, on stdout, the "Measured" bullet of DESIGN.md section 4.3
  python tools/exp_lake_stats.py --one 4096
        two device calls at that size, the first capturing the level loop, the second replaying it (for rocprofv3
        --kernel-trace --stats)

The bench's random field (ws_random_field_device), seeds from find_local_minima, u16 weights.  Legs, per size:
  stats_ms         (a) ws_merge_tree_stats_device, tree and records left in HBM
  tree_ms          (b) ws_merge_tree_device of the same field; stats_minus_tree_ms = (a) - (b): what the catalogue costs
  route_ms         (c) today's route, up to --route-max only: merge_tree with labels, transform_history of every level before a death
                   level (and the last), and per plane torch scatter reductions by label on the device; its records must equal (a)'s
--tree-runs: results of tools/exp_merge_tree.py written by alternate runs of two checkouts (LABEL parent or branch), copied into
the JSON as the evidence that merge_tree itself did not move.  Wall-clock milliseconds, median of --reps (7), the first call of
each leg not counted (graph capture, buffers)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALIVE = 0xFFFFFFFF


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


def route_records(torch, eng, img, seeds, v):
    """The records by the calls the library had before merge_tree_stats: (n_seeds + 1, 12) int64 on the device, columns sum_w, sum_wr,
    sum_wc, sum_r, sum_c, r_min, r_max, c_min, c_max, w_min, w_max, peak_pixel.  v: the weights as an int64 plane on the device."""
    h, w = img.shape
    tree, labels = eng.merge_tree(img, seeds, want_labels=True)
    n = tree.shape[0]
    death = tree[:, 1].long() & 0xFFFFFFFF
    exists = tree[:, 3] > 0
    before = torch.where(death == ALIVE, torch.full_like(death, 254), death - 1)
    before[~exists] = -2
    before[0] = 254
    levels = sorted(int(x) for x in torch.unique(before[before >= 0]).tolist())
    planes = eng.transform_history(img, seeds, levels=levels, merging=True)
    idx = torch.arange(h * w, device=img.device, dtype=torch.int64)
    row, col = idx // w, idx % w
    val = v.reshape(-1)
    packed = (val << 32) | (0xFFFFFFFF - idx)
    big = torch.iinfo(torch.int64).max
    out = torch.zeros((n, 12), dtype=torch.int64, device=img.device)
    for k, L in enumerate(levels):
        lab = planes[k].reshape(-1).long()
        rec = torch.zeros((n, 12), dtype=torch.int64, device=img.device)
        for j, x in enumerate((val, val * row, val * col, row, col)):
            rec[:, j].index_add_(0, lab, x)
        for j, x in ((5, row), (7, col), (9, val)):
            rec[:, j] = torch.full((n,), big, dtype=torch.int64, device=img.device).scatter_reduce_(0, lab, x, "amin")
        for j, x in ((6, row), (8, col)):
            rec[:, j] = torch.zeros(n, dtype=torch.int64, device=img.device).scatter_reduce_(0, lab, x, "amax")
        peak = torch.zeros(n, dtype=torch.int64, device=img.device).scatter_reduce_(0, lab, packed, "amax")
        rec[:, 10] = peak >> 32
        rec[:, 11] = 0xFFFFFFFF - (peak & 0xFFFFFFFF)
        mine = before == L
        out[mine] = rec[mine]
    none = torch.tensor([0, 0, 0, 0, 0, ALIVE, 0, ALIVE, 0, ALIVE, 0, ALIVE], dtype=torch.int64, device=img.device)
    empty = (out[:, 5] == big) | (before == -2)
    out[empty] = none
    at0 = torch.nonzero(before == -1).reshape(-1)          # died at level 0: the seed pixel alone
    if at0.numel():
        r, c = seeds[at0 - 1, 0].long(), seeds[at0 - 1, 1].long()
        x = v[r, c]
        out[at0] = torch.stack([x, x * r, x * c, r, c, r, r, c, c, x, x, r * w + c], dim=1)
    return out, len(levels)


def records_as_columns(pkg, raw):
    rec = np.ascontiguousarray(raw).view(pkg.api.LAKE_STATS_DTYPE).reshape(-1)
    names = ("sum_w", "sum_wr", "sum_wc", "sum_r", "sum_c", "r_min", "r_max", "c_min", "c_max", "w_min", "w_max", "peak_pixel")
    return np.stack([rec[f].astype(np.int64) for f in names], axis=1)


def design_bullet(rows):
    parts = []
    for r in rows:
        t = (f"{r['size']}² ({r['seeds'] / 1e6:.2f} M seeds): tree and catalogue {r['stats_ms']} ms, tree alone {r['tree_ms']} ms, "
             f"difference {r['stats_minus_tree_ms']} ms")
        if "route_ms" in r:
            t += f"; the route through {r['route_levels']} history planes and torch scatter reductions {r['route_ms']} ms ({r['route_over_stats']}×)"
        parts.append(t)
    return "* **Measured** (`profiles/lake_stats.json`, `tools/exp_lake_stats.py`; wall ms, median of 7, one MI355X). " + ". ".join(parts) + "."


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--route-max", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lake_stats.json"))
    ap.add_argument("--one", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tree-runs", nargs="*", default=[])
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = __import__("rustronomy_watershed_amd.device", fromlist=["DeviceEngine"])
    torch.cuda.set_stream(torch.cuda.Stream(0))
    eng = dev.DeviceEngine(0)
    sync = torch.cuda.synchronize

    def weights(size):
        return torch.from_numpy(np.random.default_rng(size).integers(0, 65536, (size, size), dtype=np.uint16).view(np.int16)).to(eng.device)

    if args.one:
        img = eng.random_field(args.one, args.one, 1)
        seeds = eng.find_local_minima(img)
        wt = weights(args.one)
        tree, raw = eng.merge_tree_stats(img, seeds, weights=wt)
        sync()
        eng.merge_tree_stats(img, seeds, weights=wt, out=tree, out_stats=raw)
        sync()
        print(json.dumps({"one": args.one, "seeds": int(seeds.shape[0])}))
        return
    rows = []
    for size in args.sizes:
        img = eng.random_field(size, size, 1)
        seeds = eng.find_local_minima(img)
        wt = weights(size)
        ns = int(seeds.shape[0])
        row = {"field": "random", "size": size, "seeds": ns, "weights": "u16"}
        tree = torch.empty((ns + 1, 4), dtype=torch.int32, device=eng.device)
        raw = torch.empty((ns + 1, 9), dtype=torch.int64, device=eng.device)
        row["stats_ms"] = _timed(lambda: eng.merge_tree_stats(img, seeds, weights=wt, out=tree, out_stats=raw), args.reps, sync)
        row["tree_ms"] = _timed(lambda: eng.merge_tree(img, seeds, out=tree), args.reps, sync)
        row["stats_minus_tree_ms"] = round(row["stats_ms"] - row["tree_ms"], 3)
        row["stats_bytes"] = (ns + 1) * 72
        if size <= args.route_max:
            v = wt.long() & 0xFFFF
            got = {}

            def route():
                got["rec"], got["levels"] = route_records(torch, eng, img, seeds, v)
            row["route_ms"] = _timed(route, max(1, args.reps // 3), sync)
            row["route_levels"] = got["levels"]
            eng.merge_tree_stats(img, seeds, weights=wt, out=tree, out_stats=raw)
            sync()
            same = bool((records_as_columns(pkg, raw.cpu().numpy()) == got["rec"].cpu().numpy()).all())
            assert same, "the route's records differ from merge_tree_stats'"
            row["route_equals_stats"] = same
            row["route_over_stats"] = round(row["route_ms"] / row["stats_ms"], 1)
        print(json.dumps(row), flush=True)
        rows.append(row)
    res = {"what": "merge_tree_stats (ws_merge_tree_stats_device) vs merge_tree and vs the route through the history planes and torch "
                   "scatter reductions, wall ms (median of 7), one MI355X; see tools/exp_lake_stats.py", "rows": rows}
    runs = []
    for item in args.tree_runs:
        label, path = item.split(":", 1)
        with open(path) as f:
            runs.append({"checkout": label, "rows": [{k: r[k] for k in ("size", "tree_ms", "history_1_level_ms")} for r in json.load(f)["rows"]]})
    if runs:
        res["merge_tree_parent_vs_branch"] = {"what": "tools/exp_merge_tree.py --route-max 0 of the parent commit's checkout and of this one, run "
                                                      "alternately in this order", "runs": runs}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(design_bullet(rows))


if __name__ == "__main__":
    main()
