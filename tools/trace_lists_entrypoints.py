#!/usr/bin/env python3
"""Calls every entry point of csrc/ws_lists.hip and csrc/ws_batch.hip three times in a row (plain launches, capture, replay) on one
small case -- a 48 x 64 random field and a stack of 3 slices of 32 x 64, edge correction off and on; the cube entry points also in
two groups of slices and with the middle slice's seed list shuffled -- for a run under `rocprofv3 --kernel-trace`; and compares
two such traces launch by launch.

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/trace_lists_entrypoints.py      (WS_HIP_LIB: another build)
  tools/trace_lists_entrypoints.py --list TRACE.csv         kernel name, grid and block of every launch, in dispatch order
  tools/trace_lists_entrypoints.py --summary TRACE.csv      the distinct launches with their counts, and a SHA-256 of that whole list
  tools/trace_lists_entrypoints.py --compare A.csv B.csv                exit status 0 when both hold the same sequence
"""
import csv
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, SLICES, SLICE_H, MAXLVL, LEVELS = 48, 64, 3, 32, 254, 255


def launches(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    dims = lambda r, what: "x".join(r[f"{what}_Size_{a}"] for a in "XYZ")
    return [f"{r['Kernel_Name']} grid {dims(r, 'Grid')} block {dims(r, 'Workgroup')}" for r in rows]


def summary(path):
    import hashlib
    seq = launches(path)
    counts = {}
    for x in seq:
        counts[x] = counts.get(x, 0) + 1
    print(f"{len(seq)} launches, {len(counts)} distinct (kernel, grid, block); sha256 of the ordered list: {hashlib.sha256(chr(10).join(seq).encode()).hexdigest()}")
    for x, n in counts.items():      # in order of first appearance
        print(f"{n:8d}  {x}")


def compare(a, b):
    la, lb = launches(a), launches(b)
    first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), None)
    if first is None and len(la) == len(lb):
        print(f"identical: {len(la)} launches, {len(set(la))} distinct (kernel, grid, block)")
        return 0
    i = min(len(la), len(lb)) if first is None else first
    print(f"different: {len(la)} against {len(lb)} launches, first difference at launch {i}")
    print("  a:", la[i] if i < len(la) else "(end)")
    print("  b:", lb[i] if i < len(lb) else "(end)")
    return 1


def drive():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import __graft_entry__ as ge
    import oracle_lib as ol
    pkg = ge.load_package()
    from rustronomy_watershed_amd.device import DeviceEngine
    ffi, L = pkg._ffi, pkg._ffi.lib()
    himg = ol.random_field(H, W, 41)
    hseeds = ol.find_local_minima(himg)
    hcube = np.stack([ol.random_field(SLICE_H, W, 50 + k) for k in range(SLICES)])
    hlists = [ol.find_local_minima(s) for s in hcube]
    with torch.cuda.stream(torch.cuda.Stream(0)):
        eng = DeviceEngine(0)
        img = torch.from_numpy(himg).to(eng.device)
        seeds = torch.from_numpy(hseeds.astype(np.int32)).to(eng.device).contiguous()
        cube = torch.from_numpy(hcube).to(eng.device).contiguous()
        bseeds = torch.from_numpy(np.concatenate(hlists).astype(np.int32)).to(eng.device).contiguous()
        offs = [0] + [int(x) for x in np.cumsum([len(l) for l in hlists])]
        lakes = torch.zeros((LEVELS * (max(len(hseeds), offs[-1]) + SLICES + 1), 2), dtype=torch.int64, device=eng.device)
        for edge in (False, True):
            b = pkg.TransformBuilder.new().set_max_water_lvl(MAXLVL).set_context(eng.ctx)
            if edge:
                b.enable_edge_correction()
            seg, mer = b.build_segmenting(), b.build_merging()
            labels = eng.segment(img, seeds, edge=edge)
            keys = eng.last_arrival().clone()
            ph, pw = labels.shape
            out = torch.empty((ph, pw), dtype=torch.int32, device=eng.device)
            bout = torch.empty((SLICES, SLICE_H + 2 * edge, W + 2 * edge), dtype=torch.int32, device=eng.device)
            opt = ffi.Options(MAXLVL, int(edge))

            def from_arrival(merging):
                n = ctypes.c_size_t(0)
                o, u = np.zeros(LEVELS + 1, dtype=np.uint64), np.zeros(LEVELS, dtype=np.uint64)
                eng.ctx.check(L.ws_lists_from_arrival_device(eng.ctx.handle, merging, keys.data_ptr(), labels.data_ptr(), ph, pw, len(hseeds),
                                                             ctypes.byref(opt), lakes.data_ptr(), lakes.shape[0], ctypes.byref(n), o.ctypes.data,
                                                             u.ctypes.data))

            def begin_end():
                eng.merge_begin(img, seeds, out, edge=edge)
                eng.merge_end()

            def batch_calls(bs, hl):      # every cube entry point, device seeds bs / host lists hl
                return [
                    ("ws_transform_to_list_batch_device seg", lambda: eng.transform_to_list_batch(cube, bs, offs, merging=False, edge=edge, lakes=lakes)),
                    ("ws_transform_to_list_batch_device mer", lambda: eng.transform_to_list_batch(cube, bs, offs, merging=True, edge=edge, lakes=lakes)),
                    ("ws_transform_to_list_batch", lambda: mer.transform_to_list_cube(hcube, hl)),
                    ("ws_merge_batch_device", lambda: eng.merge_batch(cube, bs, offs, edge=edge, out=bout)),
                    ("ws_transform_history_batch_device seg", lambda: eng.transform_history_batch(cube, bs, offs, merging=False, edge=edge)),
                    ("ws_transform_history_batch_device mer", lambda: eng.transform_history_batch(cube, bs, offs, merging=True, edge=edge)),
                    ("ws_transform_history_batch", lambda: mer.transform_history_cube(hcube, hl, levels=[0, 100, 254])),
                    ("ws_merge_tree_batch_device", lambda: eng.merge_tree_batch(cube, bs, offs, edge=edge, want_labels=True)),
                    ("ws_merge_tree_batch", lambda: mer.merge_tree_cube(hcube, hl, want_labels=True)),
                    ("ws_merge_tree_stats_batch_device", lambda: eng.merge_tree_stats_batch(cube, bs, offs, edge=edge, want_labels=True)),
                    ("ws_merge_tree_stats_batch", lambda: mer.merge_tree_stats_cube(hcube, hl, want_labels=True)),
                    ("ws_segment_batch_device", lambda: eng.segment_batch(cube, bs, offs, edge=edge, out=bout)),
                ]

            calls = [
                ("ws_transform_history_device seg", lambda: eng.transform_history(img, seeds, merging=False, edge=edge)),
                ("ws_transform_history_device mer", lambda: eng.transform_history(img, seeds, merging=True, edge=edge)),
                ("ws_transform_history seg", lambda: seg.transform_history_levels(himg, hseeds)),
                ("ws_transform_history mer", lambda: mer.transform_history_levels(himg, hseeds)),
                ("ws_merge_tree_device", lambda: eng.merge_tree(img, seeds, edge=edge, want_labels=True)),
                ("ws_merge_tree", lambda: mer.merge_tree(himg, hseeds, want_labels=True)),
                ("ws_merge_tree_stats_device", lambda: eng.merge_tree_stats(img, seeds, edge=edge)),
                ("ws_merge_tree_stats", lambda: mer.merge_tree_stats(himg, hseeds)),
                ("ws_merge_device", lambda: eng.merge(img, seeds, edge=edge, out=out)),
                ("ws_merge_device_begin/_end", begin_end),
                ("ws_merge_with_hook hook", lambda: mer.transform_history(himg, hseeds)),
                ("ws_merge_with_hook final", lambda: mer.transform_final(himg, hseeds)),
                ("ws_transform_to_list_device seg", lambda: eng.transform_to_list(img, seeds, merging=False, edge=edge, lakes=lakes)),
                ("ws_transform_to_list_device mer", lambda: eng.transform_to_list(img, seeds, merging=True, edge=edge, lakes=lakes)),
                ("ws_lists_from_arrival_device seg", lambda: from_arrival(0)),
                ("ws_lists_from_arrival_device mer", lambda: from_arrival(1)),
                ("ws_transform_to_list seg", lambda: seg.transform_to_list_sparse(himg, hseeds)),
                ("ws_transform_to_list mer", lambda: mer.transform_to_list_sparse(himg, hseeds)),
            ] + batch_calls(bseeds, hlists)
            # the live-list form of the merging lists, with the threshold lowered (1: the lowest that can be set)
            live = [c for c in calls if c[0] in ("ws_transform_to_list_device mer", "ws_lists_from_arrival_device mer", "ws_transform_to_list mer",
                                                 "ws_transform_to_list_batch_device mer")]
            # the cube entry points again in two groups of slices, 2 + 1; and with the middle slice's list shuffled: the stack is
            # abandoned after a flooded group and the slice-by-slice loop takes the batch
            shuffled = [l[np.random.default_rng(5).permutation(len(l))] if k == SLICES // 2 else l for k, l in enumerate(hlists)]
            bshuffled = torch.from_numpy(np.concatenate(shuffled).astype(np.int32)).to(eng.device).contiguous()
            for phase, todo, live_min, limit in ((" ", calls, 0, 0), (" live", live, 1, 0), (" groups", batch_calls(bseeds, hlists), 0, 2 * SLICE_H * W),
                                                 (" shuffled", batch_calls(bshuffled, shuffled), 0, 2 * SLICE_H * W)):
                eng.ctx.check(L.ws_ctx_set_live_list_min_colours(eng.ctx.handle, live_min))
                eng.ctx.set_batch_pixel_limit(limit)
                for name, fn in todo:
                    launched = []
                    for _ in range(3):
                        fn()
                        torch.cuda.synchronize()
                        launched.append(eng.stats()["graph_launches"])
                    print(f"edge {int(edge)} {name}{phase.rstrip()}: graph_launches {launched}", flush=True)
            eng.ctx.check(L.ws_ctx_set_live_list_min_colours(eng.ctx.handle, 0))
            eng.ctx.set_batch_pixel_limit(0)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--list":
        print("\n".join(launches(sys.argv[2])))
    elif len(sys.argv) == 3 and sys.argv[1] == "--summary":
        summary(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        drive()
