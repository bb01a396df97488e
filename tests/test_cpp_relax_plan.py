"""Builds and runs tests/cpp/test_relax_plan.cpp: the relaxation's schedule (csrc/ws_relax_plan.hpp, plain C++) against the
launches recorded in tests/relax_plan_cases.txt, and what consecutive passes have to agree on.  No library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "test_relax_plan")


def _build():
    src = os.path.join(ROOT, "tests", "cpp", "test_relax_plan.cpp")
    deps = [src, os.path.join(ROOT, "rustronomy-watershed_amd", "csrc", "ws_relax_plan.hpp")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in deps):
        return BIN
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", BIN, src])
    return BIN


def test_relax_plan_matches_recorded_launches_and_pass_invariants():
    out = subprocess.run([_build(), os.path.join(ROOT, "tests", "relax_plan_cases.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "relax plan ok" in out.stdout
