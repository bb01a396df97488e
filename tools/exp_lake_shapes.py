"""Times merge_tree_shapes (ws_merge_tree_shapes_device) against merge_tree_stats of the same field: what the second moments cost.

  python tools/exp_lake_shapes.py [--sizes 1024 4096] [--out FILE] [--ab-runs LABEL:KIND:FILE ...]
        all legs -> JSON (default: profiles/lake_shapes.json) and, on stdout, the "Measured" bullet of DESIGN.md section 4.3.2
  python tools/exp_lake_shapes.py --one 4096
        two device calls at that size, the first capturing the level loop, the second replaying it (for rocprofv3
        --kernel-trace --stats)

The bench's random field (ws_random_field_device), seeds from find_local_minima, u16 weights.  Legs, per size:
  shapes_ms        (a) ws_merge_tree_shapes_device: tree, catalogue and second moments left in HBM
  stats_ms         (b) ws_merge_tree_stats_device of the same field; shapes_minus_stats_ms = (a) - (b): what the feature costs
  tree_ms          ws_merge_tree_device; stats_minus_tree_ms: section 4.3's own (a) - (b), next to it
The tree and the catalogue of (a) must equal (b)'s byte for byte, and every record of (a) must be its own part plus its
children's: asserted on the host from the limb sums of the pixels' roots (as tests/test_gpu_lake_shapes.py does at 1024^2) up to
--check-max (1024: there every sum is below 2^64 and the host's arithmetic stays in u64).  --ab-runs: results of
exp_lake_stats.py (KIND stats) or bench.py (KIND bench) written by alternate runs of two checkouts (LABEL parent or branch),
copied into the JSON as the evidence that the existing calls did not move.  Wall-clock milliseconds, median of --reps (7),
the first call of each leg not counted (graph capture, buffers)."""
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


def records_add_up(tree, labels, keys, wt, shapes):
    """Every record of `shapes` ((n, 12) uint64 words) is the sum over its own pixels -- those whose colour's root at their arrival
    level it is -- plus its children's records.  Exact: 20-bit pieces of the terms summed in float64 stay below 2^53 here."""
    n_px = labels.size
    size = labels.shape[1]
    parent, death = tree[:, 0].astype(np.int64), tree[:, 1].astype(np.int64)
    lab = labels.ravel().astype(np.int64)
    arr = (keys.ravel() >> 24).astype(np.int64)
    coloured = (lab != 0) & (arr != 255)
    root = np.where(coloured, lab, 0)
    while True:
        move = coloured & (death[root] <= arr)
        if not move.any():
            break
        root[move] = parent[root[move]]
    y, x = np.divmod(np.arange(n_px, dtype=np.uint64), np.uint64(size))
    v = wt.ravel().astype(np.uint64)
    ns = len(tree)
    words = shapes.astype(np.uint64).reshape(ns, 6, 2)
    assert not words[:, :, 1].any(), "a high word at a size where every sum is below 2^64"
    got = words[:, :, 0]
    dying = np.flatnonzero((death != ALIVE) & (death > 0) & (tree[:, 3] > 0))
    check = tree[:, 3] > 0
    check[0] = True
    check &= death != 0
    for j, t in enumerate((v * y * y, v * x * x, v * y * x, y * y, x * x, y * x)):      # every term below 2^40, every sum below 2^64
        want = np.zeros(ns, dtype=np.uint64)
        for shift in (0, 20, 40):
            part = np.bincount(root, weights=((t >> np.uint64(shift)) & np.uint64(0xFFFFF)).astype(np.float64), minlength=ns)
            want += part.astype(np.uint64) << np.uint64(shift)
        np.add.at(want, parent[dying], got[dying, j])
        if not (want[check] == got[check, j]).all():
            return False
    return True


def design_bullet(rows):
    parts = []
    for r in rows:
        parts.append(f"{r['size']}² ({r['seeds'] / 1e6:.2f} M seeds): tree, catalogue and shapes {r['shapes_ms']} ms, tree and catalogue "
                     f"{r['stats_ms']} ms, difference {r['shapes_minus_stats_ms']} ms (the catalogue's own over the tree: "
                     f"{r['stats_minus_tree_ms']} ms)")
    return "* **Measured** (`profiles/lake_shapes.json`, `tools/exp_lake_shapes.py`; wall ms, median of 7, one MI355X). " + ". ".join(parts) + "."


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--check-max", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lake_shapes.json"))
    ap.add_argument("--one", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ab-runs", nargs="*", default=[])
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.load_package()
    dev = __import__("rustronomy_watershed_amd.device", fromlist=["DeviceEngine"])
    torch.cuda.set_stream(torch.cuda.Stream(0))
    eng = dev.DeviceEngine(0)
    sync = torch.cuda.synchronize

    def weights(size):
        return np.random.default_rng(size).integers(0, 65536, (size, size), dtype=np.uint16)

    if args.one:
        img = eng.random_field(args.one, args.one, 1)
        seeds = eng.find_local_minima(img)
        wt = torch.from_numpy(weights(args.one).view(np.int16)).to(eng.device)
        tree, raw, shp = eng.merge_tree_shapes(img, seeds, weights=wt)
        sync()
        eng.merge_tree_shapes(img, seeds, weights=wt, out=tree, out_stats=raw, out_shapes=shp)
        sync()
        print(json.dumps({"one": args.one, "seeds": int(seeds.shape[0])}))
        return
    rows = []
    for size in args.sizes:
        img = eng.random_field(size, size, 1)
        seeds = eng.find_local_minima(img)
        hwt = weights(size)
        wt = torch.from_numpy(hwt.view(np.int16)).to(eng.device)
        ns = int(seeds.shape[0])
        row = {"field": "random", "size": size, "seeds": ns, "weights": "u16"}
        tree = torch.empty((ns + 1, 4), dtype=torch.int32, device=eng.device)
        raw = torch.empty((ns + 1, 9), dtype=torch.int64, device=eng.device)
        shp = torch.empty((ns + 1, 12), dtype=torch.int64, device=eng.device)
        tree2, raw2 = torch.empty_like(tree), torch.empty_like(raw)
        row["shapes_ms"] = _timed(lambda: eng.merge_tree_shapes(img, seeds, weights=wt, out=tree, out_stats=raw, out_shapes=shp), args.reps, sync)
        row["stats_ms"] = _timed(lambda: eng.merge_tree_stats(img, seeds, weights=wt, out=tree2, out_stats=raw2), args.reps, sync)
        same = bool((tree == tree2).all()) and bool((raw == raw2).all())
        assert same, "the tree or the catalogue of merge_tree_shapes differs from merge_tree_stats'"
        row["tree_and_stats_equal"] = same
        row["tree_ms"] = _timed(lambda: eng.merge_tree(img, seeds, out=tree2), args.reps, sync)
        row["shapes_minus_stats_ms"] = round(row["shapes_ms"] - row["stats_ms"], 3)
        row["stats_minus_tree_ms"] = round(row["stats_ms"] - row["tree_ms"], 3)
        row["shapes_bytes"] = (ns + 1) * 96
        if size <= args.check_max:
            _, _, _, labels = eng.merge_tree_shapes(img, seeds, weights=wt, out=tree, out_stats=raw, out_shapes=shp, want_labels=True)
            keys = eng.last_arrival()
            sync()
            ok = records_add_up(tree.cpu().numpy().view(np.uint32), labels.cpu().numpy().view(np.uint32), keys.cpu().numpy().view(np.uint32), hwt,
                                shp.cpu().numpy().view(np.uint64))
            assert ok, "a record is not its own part plus its children's"
            row["records_add_up"] = ok
        print(json.dumps(row), flush=True)
        rows.append(row)
    res = {"what": "merge_tree_shapes (ws_merge_tree_shapes_device) vs merge_tree_stats and merge_tree of the same field, wall ms (median "
                   "of 7), one MI355X; see tools/exp_lake_shapes.py", "rows": rows}
    runs = []
    for item in args.ab_runs:
        label, kind, path = item.split(":", 2)
        with open(path) as f:
            text = f.read()
        if kind == "stats":
            data = [{k: r[k] for k in ("size", "stats_ms", "tree_ms")} for r in json.loads(text)["rows"]]
        else:      # bench.py prints one JSON result line
            full = json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])
            data = {k: v for k, v in full.items() if isinstance(v, (int, float)) or (isinstance(v, str) and len(v) < 60)}
        runs.append({"checkout": label, "what": kind, "result": data})
    if runs:
        res["parent_vs_branch"] = {"what": "tools/exp_lake_stats.py --route-max 0 and bench.py --gpus 1 --steps 20 --warmup 20 of the parent "
                                           "commit's checkout and of this one, run alternately in this order", "runs": runs}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(design_bullet(rows))


if __name__ == "__main__":
    main()
