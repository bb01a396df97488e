"""Times tree_cut (ws_tree_cut_device) against the route a user had before it and against a render of the same bytes without walks.

  python tools/exp_tree_cut.py [--size 4096] [--out FILE]     the wall-clock legs -> JSON (default: profiles/tree_cut.json)
  python tools/exp_tree_cut.py --one cuts|floor               the calls of one leg, each twice (the second is the one to read), for
                                                              rocprofv3 --kernel-trace --stats
  python tools/exp_tree_cut.py --trace CUTS.csv FLOOR.csv     per-call kernel times from the two kernel traces, merged into the JSON

The bench's random field (ws_random_field_device), seeds from find_local_minima; the tree, the labels and the stamps from ONE
merge_tree(want_labels=True) + last_arrival(), outside every timed window.  Legs:
  (a) tree_cut         1 cut and 8 cuts, planes only and planes plus lists
  (b) torch route      what a user could do on the device before: the table by a torch loop over the tree tensor (the roots_at
                       pattern with the keep test), then the per-pixel walk as torch gathers; 1 cut and 8 cuts, planes only;
                       its planes are compared with (a)'s
  (c) floor            (kernel traces only) k_render_history of a SEGMENTING transform_history with as many levels: the same
                       8 B per pixel read and 4 B per pixel and plane written, no table, no walk
Wall-clock milliseconds around a device synchronise, median of --reps (15), the first call of each leg not counted."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29      # the copy figure the project measures bandwidth against


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


def cuts_of(pkg, n):
    C = pkg.Cut
    eight = [C(min_area=16), C(min_area=4), C(min_area=64), C(min_area=256), C(min_leaves=3), C(min_area=30, min_leaves=4),
             C(show_level=50, merge_level=50), C(show_level=254, merge_level=254)]
    return eight[:n]


def torch_route(torch, tree, keys, labels, cuts):
    """Leg (b).  The tree tensor holds u32 bits in int32: ALIVE is -1 there, and every other death level is below 255."""
    parent, death, area, leaves = (tree[:, k].long() for k in range(4))
    alive = death < 0
    death = torch.where(alive, torch.full_like(death, 1 << 32), death)
    area, leaves = area & 0xFFFFFFFF, leaves & 0xFFFFFFFF
    c = labels.long()
    t = (keys.long() >> 24) & 0xFF
    out = []
    for cut in cuts:
        keep = alive | ((area >= cut.min_area) & (leaves >= cut.min_leaves))
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


def trace_rows(path, name):
    """Durations in microseconds of every dispatch of the kernels whose name holds `name`, in dispatch order."""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if name in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, r["Kernel_Name"]))
    rows.sort()
    return [round(d, 2) for _, d, _ in rows]


def merge_trace(args):
    """--one runs every call twice: dispatch 2 i + 1 of a kernel belongs to the i-th call of the leg."""
    with open(args.out) as f:
        res = json.load(f)
    n = res["pixels"]
    cuts_csv, floor_csv = args.trace
    legs = ["cut1_planes", "cut8_planes", "cut8_planes_lists"]
    kern = {}
    for k_name in ("k_cut_check", "k_cut_table", "k_render_cut", "k_cut_compact"):
        kern[k_name] = trace_rows(cuts_csv, k_name)
    render = kern["k_render_cut"]
    assert len(render) == 2 * len(legs), render
    res["kernel_us"] = {"all_dispatches": kern}
    for i, leg in enumerate(legs):
        planes = 1 if leg.startswith("cut1") else 8
        us = render[2 * i + 1]
        res["kernel_us"][leg] = {"k_render_cut": us, "k_cut_check": kern["k_cut_check"][2 * i + 1], "k_cut_table": kern["k_cut_table"][2 * i + 1],
                                 "bytes": (8 + 4 * planes) * n, "render_TBps": round((8 + 4 * planes) * n / us / 1e6, 3),
                                 "render_share_of_copy": round((8 + 4 * planes) * n / us / 1e6 / COPY_TBS, 3)}
    hist = trace_rows(floor_csv, "k_render_history")
    assert len(hist) == 4, hist
    res["kernel_us"]["floor1_k_render_history"] = hist[1]
    res["kernel_us"]["floor8_k_render_history"] = hist[3]
    res["ratios"]["render_cut1_over_floor1_kernel"] = round(res["kernel_us"]["cut1_planes"]["k_render_cut"] / hist[1], 2)
    res["ratios"]["render_cut8_over_floor8_kernel"] = round(res["kernel_us"]["cut8_planes"]["k_render_cut"] / hist[3], 2)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["kernel_us"], indent=1))
    print(json.dumps(res["ratios"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_cut.json"))
    ap.add_argument("--one", choices=["cuts", "floor"])
    ap.add_argument("--trace", nargs=2, metavar=("CUTS_CSV", "FLOOR_CSV"))
    ap.add_argument("--reps", type=int, default=15)
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
    if args.one == "floor":
        for k in (1, 8):
            out = torch.empty((k, size, size), dtype=torch.int32, device=eng.device)
            for _ in range(2):
                eng.transform_history(img, seeds, levels=[c.show_level for c in cuts_of(pkg, 8)][:k], merging=False, out=out)
                sync()
        print(json.dumps({"one": "floor", "size": size, "seeds": ns}))
        return
    tree, labels = eng.merge_tree(img, seeds, want_labels=True)
    keys = eng.last_arrival()
    sync()
    out1 = torch.empty((1, size, size), dtype=torch.int32, device=eng.device)
    out8 = torch.empty((8, size, size), dtype=torch.int32, device=eng.device)
    c1, c8 = cuts_of(pkg, 1), cuts_of(pkg, 8)
    if args.one == "cuts":
        for fn in (lambda: eng.tree_cut(tree, keys, labels, c1, out=out1), lambda: eng.tree_cut(tree, keys, labels, c8, out=out8),
                   lambda: eng.tree_cut(tree, keys, labels, c8, out=out8, want_lakes=True)):
            for _ in range(2):
                fn()
                sync()
        print(json.dumps({"one": "cuts", "size": size, "seeds": ns}))
        return
    res = {"what": "tree_cut (ws_tree_cut_device) vs the torch route on the same device, wall ms around a synchronise (median, min, max of "
                   f"{args.reps}), one MI355X; kernel_us: per-call kernel times from rocprofv3 --kernel-trace; see tools/exp_tree_cut.py",
           "field": "random", "size": size, "pixels": size * size, "seeds": ns, "wall_ms": {}, "ratios": {}}
    w = res["wall_ms"]
    w["cut1_planes"] = _timed(lambda: eng.tree_cut(tree, keys, labels, c1, out=out1), args.reps, sync)
    w["cut8_planes"] = _timed(lambda: eng.tree_cut(tree, keys, labels, c8, out=out8), args.reps, sync)
    w["cut1_planes_lists"] = _timed(lambda: eng.tree_cut(tree, keys, labels, c1, out=out1, want_lakes=True), args.reps, sync)
    w["cut8_planes_lists"] = _timed(lambda: eng.tree_cut(tree, keys, labels, c8, out=out8, want_lakes=True), args.reps, sync)
    print(json.dumps(w), flush=True)
    got = {}
    w["torch1_planes"] = _timed(lambda: got.__setitem__(1, torch_route(torch, tree, keys, labels, c1)), max(3, args.reps // 3), sync)
    w["torch8_planes"] = _timed(lambda: got.__setitem__(8, torch_route(torch, tree, keys, labels, c8)), max(3, args.reps // 3), sync)
    res["torch_route_equals_tree_cut"] = bool(torch.equal(got[1], eng.tree_cut(tree, keys, labels, c1)) and
                                              torch.equal(got[8], eng.tree_cut(tree, keys, labels, c8)))
    _, lakes, offsets, hidden = eng.tree_cut(tree, keys, labels, c8, out=out8, want_lakes=True)
    res["regions_of_the_8_cuts"] = [int(offsets[k + 1] - offsets[k]) for k in range(8)]
    res["hidden_of_the_8_cuts"] = [int(x) for x in hidden]
    res["ratios"]["cut1_over_torch1_wall"] = round(w["cut1_planes"][0] / w["torch1_planes"][0], 4)
    res["ratios"]["cut8_over_torch8_wall"] = round(w["cut8_planes"][0] / w["torch8_planes"][0], 4)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
