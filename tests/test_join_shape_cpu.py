"""The hash join's layout, size and launch-shape arithmetic and its hint / plan keys without a GPU (csrc/join_shape.cpp: dense
applicability, region geometry, arena carving, the probe kernel's LDS budget, grid and chunk counts): tests/cpp/join_shape_tests.cpp
checks the rules' values at Q3's shapes and at their thresholds, and sweeps the invariants that keep the kernels within LDS
and their buffers. Built with g++ from host-only sources — no HIP runtime library is linked — once plainly
and once with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qurious_amd", "csrc")
ROCM = os.environ.get("ROCM", os.environ.get("ROCM_PATH", "/opt/rocm"))   # (headers only: the HIP types common.hpp names)
# join_shape.cpp calls nothing outside itself and common.hpp's inline helpers, so no HIP library is needed.
SOURCES = [os.path.join(ROOT, "tests", "cpp", "join_shape_tests.cpp"), os.path.join(CSRC, "join_shape.cpp")]
FLAGS = ["-std=c++17", "-O0", "-g", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + CSRC,
         "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections"]


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe] + SOURCES)
    needed = subprocess.run(["readelf", "-d", exe], capture_output=True, text=True, check=True).stdout
    assert "amdhip64" not in needed and "hiprtc" not in needed, needed
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout, r.stdout
    return r


def test_join_shape_logic(tmp_path):
    _build_and_run(tmp_path, "join_shape_tests", [])


def test_join_shape_logic_under_sanitizers(tmp_path):
    r = _build_and_run(tmp_path, "join_shape_tests_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
