"""Builds and runs tests/cpp/test_tile_plan.cpp: the cut of a tiled field (csrc/ws_tile_plan.hpp, plain C++) -- the places of the
ranks, the gather layout, the image window under edge correction and the dealing of a host seed list -- exhaustively over small
fields.  No library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "test_tile_plan")


def _build():
    src = os.path.join(ROOT, "tests", "cpp", "test_tile_plan.cpp")
    deps = [src, os.path.join(ROOT, "rustronomy-watershed_amd", "csrc", "ws_tile_plan.hpp")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in deps):
        return BIN
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", BIN, src])
    return BIN


def test_tile_plan_cuts_gathers_windows_and_deals_as_written_out():
    out = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tile plan ok" in out.stdout
