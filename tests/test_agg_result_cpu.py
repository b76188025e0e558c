"""The hash aggregate's host-side result logic without a GPU (csrc/agg_result.cpp: replica merge, slots -> output columns, the
device-side assembly's column descriptors): tests/cpp/agg_result_tests.cpp builds plans and slot words by hand and checks the
columns against values written out there. Built with g++ from host-only sources — no HIP runtime library is linked — once
plainly and once with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qurious_amd", "csrc")
ROCM = os.environ.get("ROCM", os.environ.get("ROCM_PATH", "/opt/rocm"))   # (headers only: the HIP types common.hpp names)
# agg_result.cpp + what it calls: pow10_i128 (expr.cpp), the dtype_* helpers (ctx.cpp). ctx.cpp's other functions call the HIP
# runtime; nothing here references them, so the linker drops their sections and no HIP library is needed.
SOURCES = [os.path.join(ROOT, "tests", "cpp", "agg_result_tests.cpp")] + [os.path.join(CSRC, f) for f in ("agg_result.cpp", "expr.cpp", "ctx.cpp")]
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


def test_agg_result_logic(tmp_path):
    _build_and_run(tmp_path, "agg_result_tests", [])


def test_agg_result_logic_under_sanitizers(tmp_path):
    r = _build_and_run(tmp_path, "agg_result_tests_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
