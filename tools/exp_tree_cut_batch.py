"""Times the cut catalogue of a cube (ws_tree_cut_catalogue_batch_device, ws_merge_tree_cut_catalogue_batch_device) against the
routes a user had before it, in the same process.

  python tools/exp_tree_cut_batch.py [--out FILE]     the wall-clock legs -> JSON (default: profiles/tree_cut_batch.json)
  python tools/exp_tree_cut_batch.py --one            every leg of the first shape with 8 cuts twice, for rocprofv3 --kernel-trace --stats

Shapes: 16 x 1024^2 and 8 x 2048^2 random slices (ws_random_field_device) with their own minima, the shapes of
profiles/lake_stats_batch.json; u16 weights; the 1 cut and the 8 cuts of tools/exp_tree_cut.py.  Legs:
  (B)      ws_merge_tree_cut_catalogue_batch_device: cube in, trees, catalogue, planes, lists and region records out
  (B loop) what a user had: per slice ws_merge_tree_stats_device, ws_last_arrival_device, ws_tree_cut_catalogue_device
  (A)      ws_tree_cut_catalogue_batch_device on the records, stamps and labels (B) left in HBM
  (A loop) ws_tree_cut_catalogue_device over the slices on the same inputs: the cut apart from the flood
Every loop's outputs are compared with the cube call's bit for bit.  Wall-clock milliseconds around a device synchronise, median of
--reps (15), the first call of each leg not counted."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import exp_tree_cut as base      # noqa: E402  (the cuts and the timing loop)

SHAPES = [(16, 1024, 1024), (8, 2048, 2048)]


def inputs(torch, eng, shape):
    """(cube, seeds, seed_offsets, u16 weights as int16 bits) on the device: random slices with their own minima."""
    s, h, w = shape
    cube = torch.stack([eng.random_field(h, w, 1000 + k) for k in range(s)]).contiguous()
    lists = [eng.find_local_minima(cube[k]) for k in range(s)]
    offs = [0]
    for l in lists:
        offs.append(offs[-1] + int(l.shape[0]))
    g = torch.Generator(device=eng.device).manual_seed(7)
    wt = torch.randint(-32768, 32768, shape, dtype=torch.int16, device=eng.device, generator=g)
    return cube, torch.cat(lists).contiguous(), offs, wt


def legs_of(torch, eng, pkg, cube, seeds, offs, wt, n_cuts):
    cuts = base.cuts_of(pkg, n_cuts)
    s = cube.shape[0]
    first = [offs[k] + k for k in range(s + 1)]
    res = eng.merge_tree_cut_catalogue_batch(cube, seeds, offs, cuts, weights=wt, want_labels=True, want_keys=True)
    torch.cuda.synchronize()
    tree, stats, keys, labels = res["tree"], res["stats"], res["keys"], res["labels"]

    def b_call():
        return eng.merge_tree_cut_catalogue_batch(cube, seeds, offs, cuts, weights=wt)

    def b_loop():
        out = []
        for k in range(s):
            t, st, lab = eng.merge_tree_stats(cube[k], seeds[offs[k]:offs[k + 1]], weights=wt[k], want_labels=True)
            out.append(eng.tree_cut_catalogue(t, eng.last_arrival(), lab, cuts, wt[k], stats=st))
        return out

    def a_call():
        return eng.tree_cut_catalogue_batch(tree, keys, labels, offs, cuts, weights=wt, stats=stats)

    def a_loop():
        return [eng.tree_cut_catalogue(tree[first[k]:first[k + 1]], keys[k], labels[k], cuts, wt[k], stats=stats[first[k]:first[k + 1]]) for k in range(s)]

    # the loops' outputs are the cube calls', bit for bit
    a, k = a_call(), n_cuts
    torch.cuda.synchronize()
    for name, loop in (("A", a_loop()), ("B", b_loop())):
        for i, one in enumerate(loop):
            lo, hi = int(a[3][i * k]), int(a[3][(i + 1) * k])
            assert torch.equal(a[0][i], one[0]) and torch.equal(a[1][lo:hi], one[1]) and torch.equal(a[2][lo:hi], one[2]), (name, i)
            assert (a[5][i * k:(i + 1) * k] == one[5]).all(), (name, i)
    assert torch.equal(res["planes"], a[0]) and torch.equal(res["lakes"], a[1]) and torch.equal(res["region_stats"], a[2])
    return {"B": b_call, "B_loop": b_loop, "A": a_call, "A_loop": a_loop}, int(a[1].shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_cut_batch.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--one", action="store_true")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build_hip()
    pkg = ge.load_package()
    from rustronomy_watershed_amd.device import DeviceEngine
    with torch.cuda.stream(torch.cuda.Stream(0)):
        eng = DeviceEngine(0)
        if args.one:
            cube, seeds, offs, wt = inputs(torch, eng, SHAPES[0])
            legs, _ = legs_of(torch, eng, pkg, cube, seeds, offs, wt, 8)
            for name in ("B", "B_loop", "A", "A_loop"):
                for _ in range(2):
                    legs[name]()
                    torch.cuda.synchronize()
            return
        out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "unit": "ms, wall around a synchronise: median [min, max]", "shapes": {}}
        for shape in SHAPES:
            cube, seeds, offs, wt = inputs(torch, eng, shape)
            entry = {"seeds": offs[-1]}
            for n_cuts in (1, 8):
                legs, records = legs_of(torch, eng, pkg, cube, seeds, offs, wt, n_cuts)
                row = {"records": records}
                for name, fn in legs.items():
                    med, lo, hi = base._timed(fn, args.reps, torch.cuda.synchronize)
                    row[name] = {"median": med, "min": lo, "max": hi}
                row["B_loop_over_B"] = round(row["B_loop"]["median"] / row["B"]["median"], 2)
                row["A_loop_over_A"] = round(row["A_loop"]["median"] / row["A"]["median"], 2)
                entry[f"cuts{n_cuts}"] = row
                print(shape, n_cuts, json.dumps(row), flush=True)
            out["shapes"]["x".join(str(x) for x in shape)] = entry
            del cube, seeds, wt, legs
            torch.cuda.empty_cache()
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
