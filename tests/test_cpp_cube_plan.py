"""Builds and runs tests/cpp/test_cube_plan.cpp: the host arithmetic of the cube front end (csrc/ws_cube_plan.hpp, plain C++) -- a
strided view's extent and span, the runs of the stacked minima, offsets summed across runs -- as a stand-alone program under the
address and undefined-behaviour sanitizers.  No library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "test_cube_plan")


def _build():
    src = os.path.join(ROOT, "tests", "cpp", "test_cube_plan.cpp")
    deps = [src, os.path.join(ROOT, "rustronomy-watershed_amd", "csrc", "ws_cube_plan.hpp")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in deps):
        return BIN
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", BIN, src])
    return BIN


def test_cube_plan_extents_runs_and_offsets():
    out = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cube plan ok" in out.stdout
