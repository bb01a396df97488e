"""Times tree_cut with catalogue thresholds (ws_tree_cut_stats_device) against ws_tree_cut_device and against the torch route.

  python tools/exp_tree_cut_stats.py [--size 4096] [--out FILE]   the wall-clock legs -> JSON (default: profiles/tree_cut_stats.json)
  python tools/exp_tree_cut_stats.py --one cuts                   the calls of legs (a) and (b), each twice (the second is the one to
                                                                  read), for rocprofv3 --kernel-trace --stats under the tuning build:
                                                                  WS_CUT_TABLE_FROM_RECORDS=0 packs keys whatever the tables, =1 has
                                                                  the table kernel read the 72-byte records itself (the direct form);
                                                                  the product takes the records for one catalogue table, else the keys
  python tools/exp_tree_cut_stats.py --trace KEYS.csv [DIRECT.csv]  per-call kernel times from those traces, merged into the JSON

The field of tools/exp_tree_cut.py (ws_random_field_device, seeds from find_local_minima); the tree, the catalogue (the image is the
weight plane), the labels and the stamps from ONE merge_tree_stats(want_labels=True) + last_arrival(), outside every timed window.
The thresholds are quantiles of the dead nodes' own sum_w, w_max, depth -- and, for leg (b), of their areas at the SAME quantiles, so
that both legs drop a similar share of the nodes; the shares are reported.  Legs:
  (a) the new call     1 cut and 8 cuts with catalogue thresholds (8 tables), planes only, and 8 cuts with lists
  (b) the floor        ws_tree_cut_device, 1 and 8 cuts by min_area (8 tables: where two quantiles give one area, min_leaves = 1 or the
                       next area make a table of their own): what the render and a 16-byte-a-step table cost
  (c) torch route      the table by the roots_at loop with the catalogue keep test, then the walk as gathers; planes compared with (a)
Wall-clock milliseconds around a device synchronise, median of --reps (15), the first call of each leg not counted."""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUANTILES = [0.5, 0.25, 0.75, 0.9, 0.5, 0.75, 0.5, 0.75]      # of the dead nodes, per cut
WHICH = ["sum_w", "sum_w", "sum_w", "sum_w", "w_max", "w_max", "depth", "depth"]


def _timed(fn, reps, sync):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)


def node_values(np, tree, stats):
    """Per node, from the downloaded tensors: dead, area, sum_w, w_max, depth (numpy)."""
    t = tree.cpu().numpy().view(np.uint32)
    s = stats.cpu().numpy()
    death, area = t[:, 1], t[:, 2].astype(np.int64)
    dead = death != 0xFFFFFFFF
    sum_w = s[:, 0].view(np.uint64)
    w_min, w_max = (s[:, 7] & 0xFFFFFFFF), ((s[:, 7] >> 32) & 0xFFFFFFFF)
    d = death.astype(np.int64)
    depth = np.where(dead & (d > w_min), d - w_min, 0)
    return dead, {"area": area, "sum_w": sum_w, "w_max": w_max, "depth": depth}


def make_cuts(np, pkg, tree, stats):
    """(catalogue cuts, area cuts, the share of dead nodes each drops)."""
    dead, v = node_values(np, tree, stats)
    cat, plain, shares = [], [], []
    for q, which in zip(QUANTILES, WHICH):
        x = int(np.quantile(v[which][dead], q, method="lower")) + 1      # drops the nodes up to the quantile
        a = int(np.quantile(v["area"][dead], q, method="lower")) + 1
        cat.append(pkg.Cut(**{"min_" + which: x}))
        leaves = 0      # areas are small integers and quantiles collide: min_leaves = 1 keeps what min_leaves = 0 keeps and is a table
        while pkg.Cut(min_area=a, min_leaves=leaves) in plain:      # of its own; after that the next area
            a, leaves = (a, 1) if leaves == 0 else (a + 1, 0)
        plain.append(pkg.Cut(min_area=a, min_leaves=leaves))
        shares.append({"cut": which, "threshold": x, "dropped_share": round(float((v[which][dead] < x).mean()), 4), "min_area": a,
                       "dropped_share_by_area": round(float((v["area"][dead] < a).mean()), 4)})
    return cat, plain, shares


def torch_route(torch, tree, stats, keys, labels, cuts):
    """Leg (c).  The tree tensor holds u32 bits in int32 (ALIVE is -1), the catalogue u64 / packed u32 bits in int64."""
    parent, death, area, leaves = (tree[:, k].long() for k in range(4))
    alive = death < 0
    death = torch.where(alive, torch.full_like(death, 1 << 32), death)
    area, leaves = area & 0xFFFFFFFF, leaves & 0xFFFFFFFF
    sum_w = stats[:, 0]      # below 2^63 on this field: the signed compare is the unsigned one
    w_min, w_max = stats[:, 7] & 0xFFFFFFFF, (stats[:, 7] >> 32) & 0xFFFFFFFF
    depth = torch.where(~alive & (death > w_min), death - w_min, torch.zeros_like(death))
    c = labels.long()
    t = (keys.long() >> 24) & 0xFF
    out = []
    for cut in cuts:
        keep = alive | ((area >= cut.min_area) & (leaves >= cut.min_leaves) & (sum_w >= cut.min_sum_w) & (w_max >= cut.min_w_max) &
                        (depth >= cut.min_depth))
        node = torch.arange(parent.numel(), device=tree.device)
        while True:
            gone = ~keep[node]
            if not bool(gone.any()):
                break
            node = torch.where(gone, parent[node], node)
        shown = (c != 0) & (t <= cut.show_level)
        until = torch.clamp(t, min=cut.merge_level)
        at = node[c]
        while True:
            go = shown & (death[at] <= until)
            if not bool(go.any()):
                break
            at = torch.where(go, parent[at], at)
        out.append(torch.where(shown, at, torch.zeros_like(at)).int())
    return torch.stack(out)


def trace_rows(path):
    """{kernel: [microseconds of every dispatch, in dispatch order]} for the kernels of a call; the table kernels by their source."""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            m = re.search(r"k_cut_table<[^0-9>]*(\d)", name)
            if m:
                key = "k_cut_table<%s>" % ("tree", "keys", "records")[int(m.group(1))]
            else:
                key = next((k for k in ("k_cut_keys", "k_cut_check", "k_render_cut") if k in name), None)
            if key:
                rows.append((int(r["Start_Timestamp"]), key, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    out = {}
    for _, key, us in rows:
        out.setdefault(key, []).append(round(us, 2))
    return out


ONE_LEGS = ["stats1", "stats8", "plain1", "plain8"]      # the order of --one cuts; every call twice


def merge_trace(args):
    with open(args.out) as f:
        res = json.load(f)
    k = trace_rows(args.trace[0])
    res["kernel_us"] = {"all_dispatches_keys_form": k}
    second = lambda rows, i: rows[2 * i + 1]
    res["kernel_us"]["k_cut_keys"] = {"stats1": second(k["k_cut_keys"], 0), "stats8": second(k["k_cut_keys"], 1)}
    res["kernel_us"]["table_keys_form"] = {"stats1": second(k["k_cut_table<keys>"], 0), "stats8": second(k["k_cut_table<keys>"], 1)}
    res["kernel_us"]["table_parent_form"] = {"plain1": second(k["k_cut_table<tree>"], 0), "plain8": second(k["k_cut_table<tree>"], 1)}
    res["kernel_us"]["k_render_cut"] = dict(zip(ONE_LEGS, (second(k["k_render_cut"], i) for i in range(4))))
    ts8, tp8 = res["tables"]["stats8"], res["tables"]["plain8"]      # (equal quantiles of a quantity with few values share a table)
    per = {"keys_1_table": res["kernel_us"]["table_keys_form"]["stats1"], "keys_per_table_of_8": round(res["kernel_us"]["table_keys_form"]["stats8"] / ts8, 2),
           "parent_1_table": res["kernel_us"]["table_parent_form"]["plain1"],
           "parent_per_table_of_8": round(res["kernel_us"]["table_parent_form"]["plain8"] / tp8, 2)}
    if len(args.trace) > 1:
        d = trace_rows(args.trace[1])
        res["kernel_us"]["all_dispatches_direct_form"] = d
        res["kernel_us"]["table_direct_form"] = {"stats1": second(d["k_cut_table<records>"], 0), "stats8": second(d["k_cut_table<records>"], 1)}
        per["direct_1_table"] = res["kernel_us"]["table_direct_form"]["stats1"]
        per["direct_per_table_of_8"] = round(res["kernel_us"]["table_direct_form"]["stats8"] / ts8, 2)
    res["table_us_per_table"] = per
    res["ratios"]["table_keys_over_parent_1"] = round(per["keys_1_table"] / per["parent_1_table"], 2)
    res["ratios"]["table_keys_over_parent_per_table_of_8"] = round(per["keys_per_table_of_8"] / per["parent_per_table_of_8"], 2)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["table_us_per_table"]), json.dumps(res["kernel_us"]["k_cut_keys"]), json.dumps(res["ratios"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_cut_stats.json"))
    ap.add_argument("--one", choices=["cuts"])
    ap.add_argument("--trace", nargs="+", metavar="CSV")
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    if args.trace:
        return merge_trace(args)
    import numpy as np
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = __import__("rustronomy_watershed_amd.device", fromlist=["DeviceEngine"])
    torch.cuda.set_stream(torch.cuda.Stream(0))
    eng = dev.DeviceEngine(0)
    sync = torch.cuda.synchronize
    size = args.size
    img = eng.random_field(size, size, 1)
    seeds = eng.find_local_minima(img)
    ns = int(seeds.shape[0])
    tree, stats, labels = eng.merge_tree_stats(img, seeds, want_labels=True)
    keys = eng.last_arrival()
    sync()
    cat8, plain8, shares = make_cuts(np, pkg, tree, stats)
    cat1, plain1 = cat8[:1], plain8[:1]
    out1 = torch.empty((1, size, size), dtype=torch.int32, device=eng.device)
    out8 = torch.empty((8, size, size), dtype=torch.int32, device=eng.device)
    legs = {"stats1": lambda: eng.tree_cut(tree, keys, labels, cat1, out=out1, stats=stats),
            "stats8": lambda: eng.tree_cut(tree, keys, labels, cat8, out=out8, stats=stats),
            "plain1": lambda: eng.tree_cut(tree, keys, labels, plain1, out=out1),
            "plain8": lambda: eng.tree_cut(tree, keys, labels, plain8, out=out8)}
    if args.one == "cuts":
        for leg in ONE_LEGS:
            for _ in range(2):
                legs[leg]()
                sync()
        print(json.dumps({"one": "cuts", "size": size, "seeds": ns, "lib": os.environ.get("WS_HIP_LIB", "product"),
                          "from_records": os.environ.get("WS_CUT_TABLE_FROM_RECORDS")}))
        return
    res = {"what": "tree_cut with catalogue thresholds (ws_tree_cut_stats_device) vs ws_tree_cut_device by min_area at the same quantiles and "
                   f"vs the torch route on the same device, wall ms around a synchronise (median, min, max of {args.reps}), one MI355X; "
                   "kernel_us: per-call kernel times from rocprofv3 --kernel-trace; see tools/exp_tree_cut_stats.py",
           "field": "random", "size": size, "pixels": size * size, "seeds": ns, "cuts": shares,
           "tables": {"stats8": len(set(cat8)), "plain8": len(set(plain8))}, "wall_ms": {}, "ratios": {}}
    w = res["wall_ms"]
    for leg in ONE_LEGS:
        w[leg] = _timed(legs[leg], args.reps, sync)
    w["stats8_lists"] = _timed(lambda: eng.tree_cut(tree, keys, labels, cat8, out=out8, stats=stats, want_lakes=True), args.reps, sync)
    w["plain8_lists"] = _timed(lambda: eng.tree_cut(tree, keys, labels, plain8, out=out8, want_lakes=True), args.reps, sync)
    print(json.dumps(w), flush=True)
    got = {}
    w["torch1"] = _timed(lambda: got.__setitem__(1, torch_route(torch, tree, stats, keys, labels, cat1)), max(3, args.reps // 3), sync)
    w["torch8"] = _timed(lambda: got.__setitem__(8, torch_route(torch, tree, stats, keys, labels, cat8)), max(3, args.reps // 3), sync)
    res["torch_route_equals_tree_cut"] = bool(torch.equal(got[1], legs["stats1"]()) and torch.equal(got[8], legs["stats8"]()))
    _, lakes, offsets, hidden = eng.tree_cut(tree, keys, labels, cat8, out=out8, stats=stats, want_lakes=True)
    res["regions_of_the_8_cuts"] = [int(offsets[k + 1] - offsets[k]) for k in range(8)]
    _, lakes, offsets, hidden = eng.tree_cut(tree, keys, labels, plain8, out=out8, want_lakes=True)
    res["regions_of_the_8_area_cuts"] = [int(offsets[k + 1] - offsets[k]) for k in range(8)]
    r = res["ratios"]
    r["stats1_over_plain1_wall"] = round(w["stats1"][0] / w["plain1"][0], 3)
    r["stats8_over_plain8_wall"] = round(w["stats8"][0] / w["plain8"][0], 3)
    r["stats1_over_torch1_wall"] = round(w["stats1"][0] / w["torch1"][0], 4)
    r["stats8_over_torch8_wall"] = round(w["stats8"][0] / w["torch8"][0], 4)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
