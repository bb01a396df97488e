"""Times merge_tree from the planes of a finished transform (ws_merge_tree_from_arrival_device) against ws_merge_tree_device, and
merge_tree of a field in row blocks over local groups (ws_merge_tree_tiled_device) against the single-context call.

  python tools/exp_merge_tree_tiled.py [--sizes 1024 4096] [--tiled-size 4096] [--ranks 2 4] [--out FILE]
                                        all legs -> JSON (default: profiles/merge_tree_tiled.json) and, on stdout, the "Measured"
                                        bullet of DESIGN.md section 4.2.2
  python tools/exp_merge_tree_tiled.py --one 4096
                                        three arrival calls at that size (for rocprofv3 --kernel-trace --stats: k_seed_pixels)

The bench's random field (ws_random_field_device), seeds from find_local_minima.  Legs:
  arrival_ms           ws_merge_tree_from_arrival_device on the stamps and labels a prior ws_segment_device left (copies of them)
  tree_ms              ws_merge_tree_device of the same field on the same context: the flood and the same level loop
  arrival_stats_ms / tree_stats_ms   the same with the u16 catalogue
  tiled_ms             ws_merge_tree_tiled_device, R local ranks on ONE device: the overhead of the route, not a speed-up
  flood_tiled_ms       ws_segment_tiled_device alone on the same blocks (the first part of the tiled call)
  gathers_ms           tiled_ms - flood_tiled_ms - arrival_ms: the two gathers onto rank 0 (and its buffers' first touch), by subtraction
Wall-clock milliseconds, median of --reps (7), the first call of each leg not counted (graph capture, buffers).  No multi-GPU
figure: the ranks of a local group share the one device here."""
import argparse
import json
import os
import statistics
import sys
import time

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


def design_bullet(rows, tiled):
    parts = [f"{r['size']}² ({r['seeds'] / 1e6:.2f} M seeds): from the planes {r['arrival_ms']} ms against {r['tree_ms']} ms for ws_merge_tree_device, "
             f"with the catalogue {r['arrival_stats_ms']} against {r['tree_stats_ms']} ms" for r in rows]
    parts += [f"{t['size']}² in {t['ranks']} row blocks on one device: {t['tiled_ms']} ms (flood {t['flood_tiled_ms']}, gathers {t['gathers_ms']}, "
              f"{t['gather_share']:.0%} of the call) against {t['tree_ms']} ms on one context" for t in tiled]
    return ("* **Measured** (`profiles/merge_tree_tiled.json`, `tools/exp_merge_tree_tiled.py`; wall ms, median of 7, one MI355X; no multi-GPU "
            "figure exists). " + ". ".join(parts) + ".")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--tiled-size", type=int, default=4096)
    ap.add_argument("--ranks", type=int, nargs="*", default=[2, 4])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_tree_tiled.json"))
    ap.add_argument("--one", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.load_package()
    dev = __import__("rustronomy_watershed_amd.device", fromlist=["DeviceEngine"])
    grp = __import__("rustronomy_watershed_amd.group", fromlist=["Group"])
    torch.cuda.set_stream(torch.cuda.Stream(0))
    eng = dev.DeviceEngine(0)
    sync = torch.cuda.synchronize

    def planes_of(img, seeds):
        labels = eng.segment(img, seeds).clone()
        return eng.last_arrival().clone(), labels

    if args.one:
        img = eng.random_field(args.one, args.one, 1)
        seeds = eng.find_local_minima(img)
        keys, labels = planes_of(img, seeds)
        for _ in range(3):
            eng.merge_tree_from_arrival(keys, labels, int(seeds.shape[0]))
            sync()
        print(json.dumps({"one": args.one, "seeds": int(seeds.shape[0])}))
        return
    rows, tiled = [], []
    for size in args.sizes:
        img = eng.random_field(size, size, 1)
        seeds = eng.find_local_minima(img)
        ns = int(seeds.shape[0])
        keys, labels = planes_of(img, seeds)
        wt = torch.randint(0, 32768, (size, size), dtype=torch.int16, device=eng.device)
        out = torch.empty((ns + 1, 4), dtype=torch.int32, device=eng.device)
        out_stats = torch.empty((ns + 1, 9), dtype=torch.int64, device=eng.device)
        row = {"field": "random", "size": size, "seeds": ns}
        row["arrival_ms"] = _timed(lambda: eng.merge_tree_from_arrival(keys, labels, ns), args.reps, sync)
        row["tree_ms"] = _timed(lambda: eng.merge_tree(img, seeds, out=out), args.reps, sync)
        row["arrival_stats_ms"] = _timed(lambda: eng.merge_tree_from_arrival(keys, labels, ns, weights=wt, want_stats=True), args.reps, sync)
        row["tree_stats_ms"] = _timed(lambda: eng.merge_tree_stats(img, seeds, weights=wt, out=out, out_stats=out_stats), args.reps, sync)
        a = eng.merge_tree_from_arrival(keys, labels, ns, weights=wt, want_stats=True)
        b = eng.merge_tree_stats(img, seeds, weights=wt)
        row["arrival_equals_tree"] = bool((a[0] == b[0]).all() and (a[1] == b[1]).all())
        print(json.dumps(row), flush=True)
        rows.append(row)
        if size != args.tiled_size:
            continue
        for ranks in args.ranks:
            g = grp.Group.local(ranks)
            blocks, spans, keep = g.make_blocks(size, lambda lo, hi, rank: img[lo:hi].contiguous(), seeds)
            t = {"field": "random", "size": size, "seeds": ns, "ranks": ranks, "devices": 1}
            got = {}

            def call():
                got["tree"] = g.merge_tree_tiled_device(size, size, ns, blocks, device=eng.device)[0]
            t["tiled_ms"] = _timed(call, args.reps, sync)
            t["flood_tiled_ms"] = _timed(lambda: g.segment_tiled_device(size, size, ns, blocks), args.reps, sync)
            t["arrival_ms"], t["tree_ms"] = row["arrival_ms"], row["tree_ms"]
            t["gathers_ms"] = round(t["tiled_ms"] - t["flood_tiled_ms"] - t["arrival_ms"], 3)
            t["gather_share"] = round(t["gathers_ms"] / t["tiled_ms"], 3)
            t["gathered_bytes"] = 8 * size * size
            t["tiled_equals_tree"] = bool((got["tree"] == eng.merge_tree(img, seeds)).all())
            print(json.dumps(t), flush=True)
            tiled.append(t)
            g.close()
    res = {"what": "merge_tree from arrival planes (ws_merge_tree_from_arrival_device) vs ws_merge_tree_device, and merge_tree of a field "
                   "in row blocks over local groups on ONE device (ws_merge_tree_tiled_device) vs the single-context call; wall ms (median of "
                   "7), one MI355X; no multi-GPU figure exists; see tools/exp_merge_tree_tiled.py", "rows": rows, "tiled": tiled}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(design_bullet(rows, tiled))


if __name__ == "__main__":
    main()
