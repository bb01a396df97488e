#!/usr/bin/env python3
"""The cube front end as one call each against the per-slice routes it replaces, on the GPU.

  pre     ws_pre_processor_batch_device (f32 and f64; slice-major and channel-last cubes) against a loop of
          ws_pre_processor_device over the slices -- for a channel-last cube after the `.contiguous()` copy of each slice,
          which is what a caller had to do before the batch call took strides
  minima  ws_find_local_minima_batch_device against a loop of ws_find_local_minima_device
  host    merge_tree_cube(cube) with seeds=None (the host batch form whose minima upload_batch finds); with --parent-lib PATH
          the same in a child process on another build of the library (the parent commit's), for an A/B of item 3

Every figure: ms per call, median, min and max over --k timed windows after --warmup calls; a window holds as many calls as fill
about 20 ms between two device synchronises (host clock), and the windows of the two routes of a row alternate.
`bytes_per_s` of a pre-processor row is the call's traffic (the input read twice, by the fold and by the quantiser, and the u8
cube written once) over the call's median time: a call-level figure, not a kernel's.  Outputs of both routes are compared.
The host leg's two builds run in child processes of their own that alternate (parent, this, parent, this).
usage: bench_cube_input.py [--out FILE.json] [--k K] [--warmup W] [--legs pre,minima,host] [--shapes 16x1024x1024,...]
                           [--parent-lib PATH]
       bench_cube_input.py --one SxHxW      three f32 batch calls of each layout at that size, for rocprofv3 --kernel-trace --stats"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = "16x1024x1024,8x4096x4096,70001x8x16"

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--k", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--legs", default="pre,minima,host")
ap.add_argument("--shapes", default=SHAPES)
ap.add_argument("--parent-lib")
ap.add_argument("--one")
ap.add_argument("--child", action="store_true", help="(internal) the host leg alone on the library of WS_HIP_LIB, one JSON line per shape")
args = ap.parse_args()

import torch      # noqa: E402

import __graft_entry__ as ge      # noqa: E402

NEW = ("ws_pre_processor_batch_device", "ws_pre_processor_batch", "ws_find_local_minima_batch_device", "ws_find_local_minima_batch")
pkg = ge.load_package()
if args.child:      # maybe another build of the same ABI, from before these entry points existed
    import ctypes as _ct
    _raw = _ct.CDLL(pkg._ffi.LIB_PATH)
    for name in NEW:
        if not hasattr(_raw, name):
            pkg._ffi.SIGNATURES.pop(name, None)
L = pkg._ffi.lib()
shapes = [tuple(int(x) for x in s.split("x")) for s in (args.one or args.shapes).split(",")]
legs = args.legs.split(",")


WINDOW_MS = 20.0      # a timed window holds as many calls as fill about this long: one call of 0.1 ms measures the launch, not the work


def _window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def _summary(ts, reps):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": len(ts), "calls_per_run": reps, "samples_ms": ts}


def timed_pair(a, b, k=None, warmup=None):
    """ms per call of two routes, their windows ALTERNATING (a, b, a, b, ...) so that both see the same machine."""
    k = args.k if k is None else k
    reps = []
    for fn in (a, b):
        for _ in range(args.warmup if warmup is None else warmup):
            fn()
        reps.append(max(1, min(200, int(WINDOW_MS / max(_window(fn, 1), 1e-3)))))
    ta, tb = [], []
    for _ in range(k):
        ta.append(_window(a, reps[0]))
        tb.append(_window(b, reps[1]))
    return _summary(ta, reps[0]), _summary(tb, reps[1])


def timed(fn, k=None, warmup=None):
    for _ in range(args.warmup if warmup is None else warmup):
        fn()
    reps = max(1, min(200, int(WINDOW_MS / max(_window(fn, 1), 1e-3))))
    return _summary([_window(fn, reps) for _ in range(args.k if k is None else k)], reps)


def verdict(one, parent):
    """not slower than the parent route beyond the parent's own run-to-run range"""
    return {"speedup": parent["median_ms"] / one["median_ms"], "not_slower": one["median_ms"] <= parent["max_ms"]}


def host_leg(ws, n, h, w):
    rng = np.random.default_rng(5)
    cube = rng.integers(0, 256, size=(n, h, w), dtype=np.uint8)
    few = n * h * w > 1 << 26
    return timed(lambda: ws.merge_tree_cube(cube), k=3 if few else None, warmup=1 if few else None)


if args.child:
    ws = pkg.TransformBuilder.new().build_merging()
    for n, h, w in shapes:
        print(json.dumps({"shape": [n, h, w], "host": host_leg(ws, n, h, w)}), flush=True)
    sys.exit(0)

import importlib      # noqa: E402

dev = importlib.import_module("rustronomy_watershed_amd.device")
torch.cuda.set_stream(torch.cuda.Stream(0))
eng = dev.DeviceEngine(0)
H = eng.ctx.handle
results = []


def check(rc):
    eng.ctx.check(rc)


def field(n, h, w, dtype, channel_last):
    g = torch.Generator(device=eng.device).manual_seed(7)
    store = torch.randn((h, w, n) if channel_last else (n, h, w), generator=g, device=eng.device, dtype=torch.float32)
    store = store * 100.0
    return store.to(dtype)


for n, h, w in shapes:
    hw = n * h * w
    many = n > 1024                      # a loop of tens of thousands of calls: fewer repetitions
    kk, ww = (3, 1) if many else (None, None)
    if "pre" in legs or args.one:
        for dtype, code, es in ((torch.float32, 0, 4), (torch.float64, 1, 8)):
            if args.one and code:
                continue
            for channel_last in (False, True):
                t = field(n, h, w, dtype, channel_last)
                view = t.movedim(2, 0) if channel_last else t
                ss, rs, cs = view.stride()
                out = torch.empty((n, h, w), dtype=torch.uint8, device=eng.device)

                def one():
                    check(L.ws_pre_processor_batch_device(H, t.data_ptr(), code, n, h, w, ss, rs, cs, 254, out.data_ptr(), None, None))

                if args.one:
                    for _ in range(3):
                        one()
                    torch.cuda.synchronize()
                    continue
                out2 = torch.empty_like(out)

                def loop():
                    for k in range(n):
                        src = view[k].contiguous()      # (already contiguous in a slice-major cube: no copy)
                        check(L.ws_pre_processor_device(H, src.data_ptr(), code, h * w, 254, out2[k].data_ptr()))

                a, b = timed_pair(one, loop, kk, ww)
                assert torch.equal(out, out2), "the batch call and the loop disagree"
                traffic = hw * (2 * es + 1)
                r = {"leg": "pre", "shape": [n, h, w], "dtype": str(dtype).split(".")[1], "layout": "channel_last" if channel_last else "slice_major",
                     "one_call": a, "parent_route": b, "bytes": traffic, "bytes_per_s": traffic / (a["median_ms"] * 1e-3), **verdict(a, b)}
                results.append(r)
                print(json.dumps(r), flush=True)
                del t, view, out, out2
                torch.cuda.empty_cache()
    if args.one:
        continue
    if "minima" in legs:
        cube = torch.stack([eng.random_field(h, w, 1 + k % 64) for k in range(min(n, 64))])
        cube = cube[torch.arange(n, device=eng.device) % cube.shape[0]].contiguous()
        bound = ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1)
        seeds = torch.empty((n * bound, 2), dtype=torch.int32, device=eng.device)
        seeds2 = torch.empty_like(seeds)
        offs = np.zeros(n + 1, dtype=np.uintp)
        offs2 = np.zeros(n + 1, dtype=np.uintp)
        found = ctypes.c_size_t(0)

        def one():
            check(L.ws_find_local_minima_batch_device(H, cube.data_ptr(), n, h, w, w, h * w, seeds.data_ptr(), n * bound, offs.ctypes.data_as(pkg._ffi.szp),
                                                      ctypes.byref(found)))

        def loop():
            at = 0
            got = ctypes.c_size_t(0)
            for k in range(n):
                check(L.ws_find_local_minima_device(H, cube[k].data_ptr(), h, w, w, seeds2.data_ptr() + 8 * at, bound, ctypes.byref(got)))
                at += got.value
                offs2[k + 1] = at

        a, b = timed_pair(one, loop, kk, ww)
        total = int(offs[n])
        assert (offs == offs2).all() and torch.equal(seeds[:total], seeds2[:total]), "the batch call and the loop disagree"
        r = {"leg": "minima", "shape": [n, h, w], "seeds": total, "one_call": a, "parent_route": b, **verdict(a, b)}
        results.append(r)
        print(json.dumps(r), flush=True)
        del cube, seeds, seeds2
        torch.cuda.empty_cache()
    if "host" in legs:
        r = {"leg": "host_merge_tree_cube_seeds_none", "shape": [n, h, w]}
        if args.parent_lib:
            # both builds in child processes of their own, alternating (parent, this, parent, this): their windows are pooled per build
            pooled = {"parent_build": [], "this_build": []}
            for _ in range(2):
                for name, lib in (("parent_build", os.path.abspath(args.parent_lib)), ("this_build", pkg._ffi.LIB_PATH)):
                    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shapes", f"{n}x{h}x{w}", "--k", str(args.k),
                                            "--warmup", str(args.warmup)], env=dict(os.environ, WS_HIP_LIB=lib), capture_output=True, text=True, timeout=900)
                    if child.returncode != 0:
                        raise RuntimeError(f"the run of {name} failed: " + child.stderr[-2000:])
                    got = json.loads(child.stdout.strip().splitlines()[-1])["host"]
                    pooled[name] += got["samples_ms"]
                    reps = got["calls_per_run"]
            for name, ts in pooled.items():
                r[name] = _summary(ts, reps)
            r.update(verdict(r["this_build"], r["parent_build"]))
        else:
            r["this_build"] = host_leg(pkg.TransformBuilder.new().build_merging(), n, h, w)
        results.append(r)
        print(json.dumps(r), flush=True)

if args.out and not args.one:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/bench_cube_input.py", "k": args.k, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
                   "results": results}, f, indent=1)
