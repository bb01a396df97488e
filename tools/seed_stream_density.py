#!/usr/bin/env python3
"""The two seed-table builders by list density, for the rule in seed_tables().

Workload mode (no argument): on one 4096 x 4096 field, REPS segmenting transforms for each of the lists below, in this order.
Run it under `rocprofv3 --kernel-trace --output-format csv` with the -DWS_TUNING build (WS_HIP_LIB) once with
WS_SEED_STREAM=0 (k_seed_tables for every list) and once with WS_SEED_STREAM=1 (k_seed_tables_stream for every list).
  uniform_N    one seed per N pixels, uniform random, strictly increasing (N = 8, 12, 16, 24, 32, 128, 512, 4096)
  upper_N      the adversarial list: the same density, but every seed in the upper half of the plane (the rows below the
               middle), so that one window of the list-order kernel owns the quarter million empty words in front of them
`--summarise OLD_TRACE.csv NEW_TRACE.csv`: the table, microseconds per launch of the seed-table kernel of each list (the first
launch of a list left out: it is the capturing one)."""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE = 4096
REPS = 7
LISTS = [("uniform_8", 8, False), ("uniform_12", 12, False), ("uniform_16", 16, False), ("uniform_24", 24, False), ("uniform_32", 32, False), ("uniform_128", 128, False), ("uniform_512", 512, False),
         ("uniform_4096", 4096, False), ("upper_8", 8, True), ("upper_2", 2, True)]


def workload():
    import importlib
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.load_package()
    dev = importlib.import_module("rustronomy_watershed_amd.device")
    eng = dev.DeviceEngine(0)
    img = eng.random_field(SIDE, SIDE, 1)
    out = torch.empty((SIDE, SIDE), dtype=torch.int32, device=eng.device)
    g = torch.Generator(device=eng.device)
    g.manual_seed(5)
    for name, per, upper in LISTS:
        m = torch.rand(SIDE * SIDE, device=eng.device, generator=g) < 1.0 / per
        if upper:
            m[: SIDE * SIDE // 2] = False
        px = torch.nonzero(m).reshape(-1)
        seeds = torch.stack([px // SIDE, px % SIDE], dim=1).to(torch.int32).contiguous()
        for _ in range(REPS):
            eng.segment(img, seeds, out=out)
        torch.cuda.synchronize()
        print(name, "n =", int(seeds.shape[0]), flush=True)


def launches(path):
    rows = [r for r in csv.DictReader(open(path)) if "k_seed_tables" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    assert len(us) == REPS * len(LISTS), (path, len(us))
    return [us[i * REPS + 1:(i + 1) * REPS] for i in range(len(LISTS))]


def summarise(old, new):
    a, b = launches(old), launches(new)
    print("list            k_seed_tables us (min mean max)     k_seed_tables_stream us (min mean max)")
    for (name, _, _), x, y in zip(LISTS, a, b):
        print("%-14s  %7.1f %7.1f %7.1f               %7.1f %7.1f %7.1f" % (name, min(x), sum(x) / len(x), max(x), min(y), sum(y) / len(y), max(y)))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2], sys.argv[3])
    else:
        workload()
