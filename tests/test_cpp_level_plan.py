"""Builds and runs tests/cpp/test_level_plan.cpp: the per-level driver's job check and mode plan (csrc/ws_level_plan.hpp, plain
C++) against the table of modes written out in the test.  No library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "test_level_plan")


def _build():
    src = os.path.join(ROOT, "tests", "cpp", "test_level_plan.cpp")
    deps = [src, os.path.join(ROOT, "rustronomy-watershed_amd", "csrc", "ws_level_plan.hpp"), os.path.join(ROOT, "include", "ws_hip.h")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in deps):
        return BIN
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", BIN, src])
    return BIN


def test_level_plan_matches_the_table_of_modes_and_refuses_unbuilt_jobs():
    out = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "level plan ok" in out.stdout
