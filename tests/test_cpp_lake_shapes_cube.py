"""Builds and runs tests/cpp/test_lake_shapes_cube.cpp: merge_tree_shapes_cube of the C++ mirror (include/ws_watershed.hpp) against its
own merge_tree_shapes slice by slice."""
import os
import subprocess

import pytest

import __graft_entry__ as ge
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "test_lake_shapes_cube")


def _build():
    ge.build_hip()
    ol.build()
    src = os.path.join(ROOT, "tests", "cpp", "test_lake_shapes_cube.cpp")
    deps = [src, os.path.join(ROOT, "include", "ws_watershed.hpp"), os.path.join(ROOT, "include", "ws_hip.h")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in deps):
        return BIN
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", BIN, src,
                           "-L" + os.path.join(ROOT, "rustronomy-watershed_amd"), "-lws_hip",
                           "-L" + os.path.join(ROOT, "oracle", "_build"), "-lws_oracle",
                           "-Wl,-rpath,$ORIGIN/../../../rustronomy-watershed_amd",
                           "-Wl,-rpath,$ORIGIN/../../../oracle/_build"])
    return BIN


def test_cpp_lake_shapes_cube_builds():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_cpp_lake_shapes_cube_gpu():
    out = subprocess.run([_build()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "lake shapes cube ok" in out.stdout
