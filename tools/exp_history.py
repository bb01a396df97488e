"""Times transform_history for chosen levels (ws_transform_history_device / ws_transform_history) against the hook route.

  python tools/exp_history.py [--sizes 1024 2048 4096] [--out FILE]     all legs -> JSON (profiles/history.json)
  python tools/exp_history.py --one 4096                                one merging device call of all 255 levels at that size
                                                                        (for rocprofv3 --kernel-trace --stats)

Fields: the bench's random field (ws_random_field_device) and a smooth one (tests/cases.smooth_field), seeds from
find_local_minima.  Legs, per field, size and transform (segmenting / merging):
  device_all / device_8   ws_transform_history_device, 255 levels / 8 levels, planes left in HBM
  host_all / host_8       ws_transform_history, u64 planes into a fresh host array (host_all only up to 2048^2: 255 u64 planes
                          of 4096^2 are 34 GB); host_all_reused: into one array allocated (and faulted in) before the timing
  hook                    the existing route (ws_*_with_hook): every level's u64 plane to the host and a callback -- timed with
                          a callback that keeps nothing, so it never touches fresh memory (transform_history itself would keep
                          34 GB at 4096^2)
  hook_history            transform_history itself (the hook route keeping a copy of every plane), up to 2048^2
Wall-clock milliseconds, median of the repeats, the first call of each leg not counted (graph capture, buffers)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEVELS_8 = [0, 32, 64, 96, 128, 160, 192, 254]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048, 4096])
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = __import__("rustronomy_watershed_amd.device", fromlist=["DeviceEngine"])
    torch.cuda.set_stream(torch.cuda.Stream(0))
    eng = dev.DeviceEngine(0)
    sync = torch.cuda.synchronize
    if args.one:
        img = eng.random_field(args.one, args.one, 1)
        seeds = eng.find_local_minima(img)
        out = eng.transform_history(img, seeds, merging=True)
        sync()
        eng.transform_history(img, seeds, merging=True, out=out)
        sync()
        print(json.dumps({"one": args.one, "levels": 255, "seeds": int(seeds.shape[0])}))
        return
    import cases
    rows = []
    for field in ("random", "smooth"):
        for size in args.sizes:
            if field == "random":
                img = eng.random_field(size, size, 1)
            else:
                img = torch.from_numpy(cases.smooth_field(size, size, 3)).to(eng.device)
            seeds = eng.find_local_minima(img)
            himg = img.cpu().numpy()
            hseeds = seeds.cpu().numpy().astype(np.uint64)
            for merging in (False, True):
                row = {"field": field, "size": size, "seeds": int(seeds.shape[0]), "transform": "merging" if merging else "segmenting"}
                out_all = torch.empty((255, size, size), dtype=torch.int32, device=eng.device)
                row["device_all_ms"] = _timed(lambda: eng.transform_history(img, seeds, merging=merging, out=out_all), args.reps, sync)
                del out_all
                row["device_8_ms"] = _timed(lambda: eng.transform_history(img, seeds, levels=LEVELS_8, merging=merging), args.reps, sync)
                b = pkg.TransformBuilder.new()
                ws = b.build_merging() if merging else b.build_segmenting()
                if size <= 2048:
                    row["host_all_ms"] = _timed(lambda: ws.transform_history_levels(himg, hseeds), max(1, args.reps - 1), sync)
                    planes = np.empty((255,) + himg.shape, dtype=np.uint64)
                    row["host_all_reused_ms"] = _timed(lambda: ws.transform_history_levels(himg, hseeds, out=planes), args.reps, sync)
                    del planes
                    row["hook_history_ms"] = _timed(lambda: ws.transform_history(himg, hseeds), 1, sync)
                row["host_8_ms"] = _timed(lambda: ws.transform_history_levels(himg, hseeds, LEVELS_8), args.reps, sync)
                hb = pkg.TransformBuilder.new().set_wlvl_hook(lambda ctx: None)
                hws = hb.build_merging() if merging else hb.build_segmenting()
                row["hook_ms"] = _timed(lambda: hws.transform_with_hook(himg, hseeds), max(1, args.reps - 1), sync)
                print(json.dumps(row), flush=True)
                rows.append(row)
    res = {"what": "transform_history for chosen levels vs the hook route, wall ms (median), one MI355X; see tools/exp_history.py",
           "levels_8": LEVELS_8, "rows": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
