"""Times the cut catalogue (ws_tree_cut_catalogue_device) against its floor and against the route a user had before it.

  python tools/exp_tree_cut_catalogue.py [--size 4096] [--out FILE]   the wall-clock legs -> JSON (default: profiles/tree_cut_catalogue.json)
  python tools/exp_tree_cut_catalogue.py --one calls                  the calls of legs (a) and (b), each twice (the second is the one to
                                                                      read), for rocprofv3 --kernel-trace --stats
  python tools/exp_tree_cut_catalogue.py --trace KERNELS.csv          per-call kernel times from that trace, merged into the JSON
  python tools/exp_tree_cut_catalogue.py --existing FILE              the existing calls alone (tree_cut with and without lists, with and
                                                                      without catalogue thresholds): the legs a run on the parent commit
                                                                      and a run on this one are compared by

The field and the cuts of tools/exp_tree_cut.py (ws_random_field_device, seeds from find_local_minima; 1 cut and 8 cuts); the tree, the
catalogue, the labels and the stamps from ONE merge_tree_stats(want_labels=True) + last_arrival(), outside every timed window; the
image is the weight plane.  Legs:
  (a) the new call     planes, lists and records of the regions
  (b) the floor        ws_tree_cut_stats_device, planes and lists, for the same cuts in the same process
  (c) torch route      (b), then scatter reductions by label over each plane on the same device, giving the same nine columns for
                       the colours with pixels; compared with (a)'s records bit for bit
Wall-clock milliseconds around a device synchronise, median of --reps (15), the first call of each leg not counted."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import exp_tree_cut as base      # noqa: E402  (the field's cuts and the timing loop)


def torch_records(torch, planes, lakes, offsets, weights):
    """Leg (c) after the cut: per plane, the nine columns of every label by scatter reductions, then the rows of the colours the
    list holds.  Everything int64 on the device; the packed columns as DeviceEngine.merge_tree_stats returns them."""
    k, h, w = planes.shape
    n = h * w
    idx = torch.arange(n, device=planes.device, dtype=torch.int64)
    row, col = idx // w, idx % w
    v = weights.reshape(-1).long() & 0xFFFF
    peak = (v << 32) | (0xFFFFFFFF - idx)
    out = []
    for j in range(k):
        lab = planes[j].reshape(-1).long()
        m = int(lab.max()) + 1
        sums = [torch.zeros(m, dtype=torch.int64, device=lab.device).index_add_(0, lab, x) for x in (v, v * row, v * col, row, col)]
        lo = [torch.full((m,), 1 << 40, dtype=torch.int64, device=lab.device).scatter_reduce_(0, lab, x, "amin") for x in (row, col, v)]
        hi = [torch.full((m,), -1, dtype=torch.int64, device=lab.device).scatter_reduce_(0, lab, x, "amax") for x in (row, col, peak)]
        at = lakes[int(offsets[j]): int(offsets[j + 1]), 0]
        w_max, peak_px = hi[2][at] >> 32, 0xFFFFFFFF - (hi[2][at] & 0xFFFFFFFF)
        out.append(torch.stack([s[at] for s in sums] + [lo[0][at] | hi[0][at] << 32, lo[1][at] | hi[1][at] << 32, lo[2][at] | w_max << 32, peak_px], dim=1))
    return torch.cat(out)


KERNELS = ("k_cut_check", "k_cut_table", "k_render_cut", "k_cut_compact", "k_lake_init", "k_cut_measure_write", "k_cut_measure")
ONE_LEGS = ["catalogue1", "catalogue8", "floor1", "floor8"]      # the order of --one calls; every call twice


def merge_trace(args):
    """Dispatch order: a call of leg i is the (2 i + 1)-th call.  Kernels are attributed to calls by the k_cut_check that opens each."""
    with open(args.out) as f:
        res = json.load(f)
    rows = []
    with open(args.trace, newline="") as f:
        for r in csv.DictReader(f):
            name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)      # (k_cut_measure_write before k_cut_measure)
            if name:
                rows.append((int(r["Start_Timestamp"]), name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    calls = []
    for _, name, us in rows:
        if name == "k_cut_check":
            calls.append({})
        if calls:
            calls[-1][name] = round(calls[-1].get(name, 0.0) + us, 2)
    assert len(calls) == 2 * len(ONE_LEGS), len(calls)
    res["kernel_us"] = {leg: calls[2 * i + 1] for i, leg in enumerate(ONE_LEGS)}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["kernel_us"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_cut_catalogue.json"))
    ap.add_argument("--one", choices=["calls"])
    ap.add_argument("--trace", metavar="CSV")
    ap.add_argument("--existing", metavar="FILE")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--skip-torch", action="store_true", help="legs (a) and (b) alone, printed and not written: for A/B runs of two builds")
    args = ap.parse_args()
    if args.trace:
        return merge_trace(args)
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
    out = {1: torch.empty((1, size, size), dtype=torch.int32, device=eng.device), 8: torch.empty((8, size, size), dtype=torch.int32, device=eng.device)}
    cuts = {1: base.cuts_of(pkg, 1), 8: base.cuts_of(pkg, 8)}
    floor = {k: (lambda k=k: eng.tree_cut(tree, keys, labels, cuts[k], out=out[k], want_lakes=True, stats=stats)) for k in (1, 8)}
    if args.existing:
        import exp_tree_cut_stats as with_stats
        cat8, plain8, _ = with_stats.make_cuts(__import__("numpy"), pkg, tree, stats)
        legs = {"cut1_planes": lambda: eng.tree_cut(tree, keys, labels, cuts[1], out=out[1]),
                "cut8_planes": lambda: eng.tree_cut(tree, keys, labels, cuts[8], out=out[8]),
                "cut1_planes_lists": lambda: eng.tree_cut(tree, keys, labels, cuts[1], out=out[1], want_lakes=True),
                "cut8_planes_lists": lambda: eng.tree_cut(tree, keys, labels, cuts[8], out=out[8], want_lakes=True),
                "stats1": lambda: eng.tree_cut(tree, keys, labels, cat8[:1], out=out[1], stats=stats),
                "stats8": lambda: eng.tree_cut(tree, keys, labels, cat8, out=out[8], stats=stats),
                "stats8_lists": lambda: eng.tree_cut(tree, keys, labels, cat8, out=out[8], stats=stats, want_lakes=True),
                "merge_tree_stats": lambda: eng.merge_tree_stats(img, seeds)}
        res = {"what": f"the existing calls, wall ms around a synchronise (median, min, max of {args.reps}); see tools/exp_tree_cut_catalogue.py --existing",
               "size": size, "seeds": ns, "wall_ms": {name: base._timed(fn, args.reps, sync) for name, fn in legs.items()}}
        with open(args.existing, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    new = {k: (lambda k=k: eng.tree_cut_catalogue(tree, keys, labels, cuts[k], img, stats=stats, out=out[k])) for k in (1, 8)}
    if args.one == "calls":
        for fn in (new[1], new[8], floor[1], floor[8]):
            for _ in range(2):
                fn()
                sync()
        print(json.dumps({"one": "calls", "size": size, "seeds": ns}))
        return
    res = {"what": "the cut catalogue (ws_tree_cut_catalogue_device: planes, lists and region records) vs ws_tree_cut_stats_device (planes and "
                   "lists) and vs that call followed by torch scatter reductions by label, same process and device, wall ms around a synchronise "
                   f"(median, min, max of {args.reps}), one MI355X; kernel_us: per-call kernel times from rocprofv3 --kernel-trace; see "
                   "tools/exp_tree_cut_catalogue.py",
           "field": "random", "size": size, "pixels": size * size, "seeds": ns, "weights": "the image (u8)", "wall_ms": {}, "ratios": {}}
    w = res["wall_ms"]
    for k in (1, 8):
        w[f"catalogue{k}"] = base._timed(new[k], args.reps, sync)
        w[f"floor{k}"] = base._timed(floor[k], args.reps, sync)
    print(json.dumps(w), flush=True)
    if args.skip_torch:
        return
    got = {}

    def route(k):
        planes, lakes, offsets, _ = floor[k]()
        got[k] = torch_records(torch, planes, lakes, offsets, img)

    for k in (1, 8):
        w[f"torch{k}"] = base._timed(lambda k=k: route(k), max(3, args.reps // 3), sync)
    same = True
    for k in (1, 8):
        planes, lakes, region, offsets, hidden, hidden_stats = new[k]()
        sync()
        same = same and bool(torch.equal(got[k], region))
        res[f"regions_of_the_{k}_cuts"] = [int(offsets[j + 1] - offsets[j]) for j in range(k)]
    res["torch_route_equals_the_records"] = same
    r = res["ratios"]
    for k in (1, 8):
        r[f"catalogue{k}_over_floor{k}"] = round(w[f"catalogue{k}"][0] / w[f"floor{k}"][0], 3)
        r[f"catalogue{k}_over_torch{k}"] = round(w[f"catalogue{k}"][0] / w[f"torch{k}"][0], 4)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
