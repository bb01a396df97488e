"""Times merge_tree_shapes of a cube in one call (ws_merge_tree_shapes_batch_device) against the loop it replaces and against the
stats batch call: what stacking saves and what the second moments cost on a cube.

  python tools/exp_lake_shapes_batch.py [--shapes 16x1024 8x2048] [--host 16x1024] [--out FILE] [--ab-runs LABEL:KIND:FILE ...]
        all legs -> JSON (default: profiles/lake_shapes_batch.json) and, on stdout, the "Measured" bullet of DESIGN.md section 4.3.3
  python tools/exp_lake_shapes_batch.py --one 16x1024
        two device calls at that shape, the first capturing the level loop, the second replaying it (for rocprofv3
        --kernel-trace --stats)

The bench's random field per slice (ws_random_field_device), seeds from find_local_minima, u16 weights.  Legs, per shape S x N^2:
  batch_ms         (a) ws_merge_tree_shapes_batch_device: trees, catalogues and second moments of all slices left in HBM
  loop_ms          (b) ws_merge_tree_shapes_device slice by slice, with loop_min_ms / loop_max_ms: the spread of (b)'s own runs
  stats_batch_ms   (c) ws_merge_tree_stats_batch_device; batch_minus_stats_batch_ms = (a) - (c): what the shapes cost on a cube
  tree_batch_ms    ws_merge_tree_batch_device; stats_batch_minus_tree_batch_ms: section 4.3.1's difference, next to it
  host_*           (--host shapes) the host forms with given seed lists: ws_merge_tree_shapes_batch, the loop of ws_merge_tree_shapes,
                   ws_merge_tree_stats_batch
Before anything is timed the records of (a) are asserted equal to (b)'s slice by slice and its tree and catalogue to (c)'s.
--ab-runs: results of exp_lake_shapes.py (KIND shapes), exp_lake_stats.py or exp_lake_stats_batch.py (KIND stats) or bench.py (KIND bench) written by
alternate runs of two checkouts (LABEL parent or branch), copied into the JSON as the evidence that the existing calls did not
move.  Wall-clock milliseconds, median of --reps (7), the first call of each leg not counted (graph capture, buffers)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _times(fn, reps, sync):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def _timed(fn, reps, sync):
    return round(statistics.median(_times(fn, reps, sync)), 3)


def _shape(text):
    s, n = text.lower().split("x")
    return int(s), int(n)


def design_bullet(rows):
    parts = []
    for r in rows:
        text = (f"{r['slices']} × {r['size']}² ({r['seeds'] / 1e6:.2f} M seeds): one call {r['batch_ms']} ms, the loop of single calls "
                f"{r['loop_ms']} ms (its runs {r['loop_min_ms']} - {r['loop_max_ms']}), the stats batch call {r['stats_batch_ms']} ms, "
                f"difference {r['batch_minus_stats_batch_ms']} ms (the catalogue's own over the tree batch: {r['stats_batch_minus_tree_batch_ms']} ms)")
        if "host_batch_ms" in r:
            text += (f"; host forms {r['host_batch_ms']} ms against {r['host_loop_ms']} ms looped and {r['host_stats_batch_ms']} ms for the "
                     f"stats cube")
        parts.append(text)
    return ("* **Measured** (`profiles/lake_shapes_batch.json`, `tools/exp_lake_shapes_batch.py`; wall ms, median of 7, one MI355X, random "
            "fields, u16 weights). " + ". ".join(parts) + ".")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["16x1024", "8x2048"])
    ap.add_argument("--host", nargs="*", default=["16x1024"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lake_shapes_batch.json"))
    ap.add_argument("--one", default="")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ab-runs", nargs="*", default=[])
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = __import__("rustronomy_watershed_amd.device", fromlist=["DeviceEngine"])
    torch.cuda.set_stream(torch.cuda.Stream(0))
    eng = dev.DeviceEngine(0)
    sync = torch.cuda.synchronize

    def inputs(s, n):
        cube = torch.stack([eng.random_field(n, n, 1 + k) for k in range(s)]).contiguous()
        lists = [eng.find_local_minima(cube[k]) for k in range(s)]
        offs = [0] + [int(x) for x in np.cumsum([int(l.shape[0]) for l in lists])]
        hwt = np.random.default_rng(n + s).integers(0, 65536, (s, n, n), dtype=np.uint16)
        return cube, lists, torch.cat(lists).contiguous(), offs, hwt, torch.from_numpy(hwt.view(np.int16)).to(eng.device)

    if args.one:
        s, n = _shape(args.one)
        cube, lists, seeds, offs, hwt, wt = inputs(s, n)
        got = eng.merge_tree_shapes_batch(cube, seeds, offs, weights=wt)
        sync()
        eng.merge_tree_shapes_batch(cube, seeds, offs, weights=wt, out=got[0], out_stats=got[1], out_shapes=got[2])
        sync()
        print(json.dumps({"one": args.one, "seeds": offs[-1]}))
        return
    rows = []
    for text in args.shapes:
        s, n = _shape(text)
        cube, lists, seeds, offs, hwt, wt = inputs(s, n)
        total = offs[-1] + s
        row = {"field": "random", "slices": s, "size": n, "seeds": offs[-1], "weights": "u16"}
        tree = torch.empty((total, 4), dtype=torch.int32, device=eng.device)
        raw = torch.empty((total, 9), dtype=torch.int64, device=eng.device)
        shp = torch.empty((total, 12), dtype=torch.int64, device=eng.device)
        tree2, raw2 = torch.empty_like(tree), torch.empty_like(raw)
        most = max(int(l.shape[0]) for l in lists) + 1
        one = (torch.empty((most, 4), dtype=torch.int32, device=eng.device), torch.empty((most, 9), dtype=torch.int64, device=eng.device),
               torch.empty((most, 12), dtype=torch.int64, device=eng.device))

        def batch():
            eng.merge_tree_shapes_batch(cube, seeds, offs, weights=wt, out=tree, out_stats=raw, out_shapes=shp)

        def loop(check=False):
            for k in range(s):
                m = int(lists[k].shape[0]) + 1
                got = eng.merge_tree_shapes(cube[k], lists[k], weights=wt[k], out=one[0][:m], out_stats=one[1][:m], out_shapes=one[2][:m])
                if check:
                    at = offs[k] + k
                    same = all(bool((a == b[at:at + m]).all()) for a, b in zip(got, (tree, raw, shp)))
                    assert same, f"slice {k} of the batch call differs from the single call"

        batch()
        loop(check=True)
        eng.merge_tree_stats_batch(cube, seeds, offs, weights=wt, out=tree2, out_stats=raw2)
        sync()
        assert bool((tree == tree2).all()) and bool((raw == raw2).all()), "the tree or the catalogue differs from the stats batch call's"
        row["records_equal_single_calls_and_stats_batch"] = True
        row["batch_ms"] = _timed(batch, args.reps, sync)
        ts = _times(loop, args.reps, sync)
        row["loop_ms"], row["loop_min_ms"], row["loop_max_ms"] = round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)
        row["stats_batch_ms"] = _timed(lambda: eng.merge_tree_stats_batch(cube, seeds, offs, weights=wt, out=tree2, out_stats=raw2), args.reps, sync)
        row["tree_batch_ms"] = _timed(lambda: eng.merge_tree_batch(cube, seeds, offs, out=tree2), args.reps, sync)
        row["batch_minus_stats_batch_ms"] = round(row["batch_ms"] - row["stats_batch_ms"], 3)
        row["stats_batch_minus_tree_batch_ms"] = round(row["stats_batch_ms"] - row["tree_batch_ms"], 3)
        row["batch_below_loop_by_more_than_its_spread"] = bool(row["loop_ms"] - row["batch_ms"] > row["loop_max_ms"] - row["loop_min_ms"])
        row["shapes_bytes"] = total * 96
        if text in args.host:
            ws = pkg.TransformBuilder.new().build_merging()
            hcube = cube.cpu().numpy()
            hlists = [l.cpu().numpy().astype(np.uint64) for l in lists]
            want = ws.merge_tree_shapes_cube(hcube, seeds=hlists, weights=hwt)
            assert np.concatenate([x for _, _, x in want]).tobytes() == shp.cpu().numpy().tobytes(), "the host form differs from the device form"
            nothing = lambda: None
            row["host_batch_ms"] = _timed(lambda: ws.merge_tree_shapes_cube(hcube, seeds=hlists, weights=hwt), args.reps, nothing)
            row["host_loop_ms"] = _timed(lambda: [ws.merge_tree_shapes(hcube[k], hlists[k], weights=hwt[k]) for k in range(s)], args.reps, nothing)
            row["host_stats_batch_ms"] = _timed(lambda: ws.merge_tree_stats_cube(hcube, seeds=hlists, weights=hwt), args.reps, nothing)
        print(json.dumps(row), flush=True)
        rows.append(row)
    res = {"what": "merge_tree_shapes of a cube in one call (ws_merge_tree_shapes_batch(_device)) vs the loop of single calls, the stats batch "
                   "call and the tree batch call, wall ms (median of 7), one MI355X; see tools/exp_lake_shapes_batch.py", "rows": rows}
    runs = []
    for item in args.ab_runs:
        label, kind, path = item.split(":", 2)
        with open(path) as f:
            text = f.read()
        if kind == "bench":      # bench.py prints one JSON result line
            full = json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])
            data = {k: v for k, v in full.items() if isinstance(v, (int, float)) or (isinstance(v, str) and len(v) < 60)}
        else:
            keep = ("size", "slices", "plane", "shapes_ms", "stats_ms", "tree_ms", "batch_ms", "loop_ms", "tree_batch_ms")
            full = json.loads(text)      # (exp_lake_stats_batch.py calls its rows "results")
            data = [{k: r[k] for k in keep if k in r} for r in full.get("rows", full.get("results", []))]
        runs.append({"checkout": label, "what": kind, "result": data})
    if runs:
        res["parent_vs_branch"] = {"what": "tools/exp_lake_shapes.py, tools/exp_lake_stats.py --route-max 0 (single and batch) and bench.py --gpus 1 "
                                           "--steps 20 --warmup 20 of the parent commit's checkout and of this one, run alternately in this order",
                                   "runs": runs}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(design_bullet(rows))


if __name__ == "__main__":
    main()
