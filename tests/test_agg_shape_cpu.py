"""The fused aggregate's tuning policy without a GPU (csrc/agg_shape.cpp: which Decimal128 arguments travel and accumulate in
64 bits, the hot-key cache size KC, the rows per thread R, the consecutive-rows form RC, the staged scatter's PART_PR):
tests/cpp/agg_shape_tests.cpp pins the values at the catalog's Q1 and Q3 shapes and on both sides of every threshold of the
rules, each read from the source the generator emitted before the policy was moved out of plan_aggregate. Built with g++ from
agg_shape.cpp alone — no HIP runtime library is linked — once plainly and once with the address and undefined-behaviour
sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qurious_amd", "csrc")
ROCM = os.environ.get("ROCM", os.environ.get("ROCM_PATH", "/opt/rocm"))   # (headers only: the HIP types common.hpp names)
SOURCES = [os.path.join(ROOT, "tests", "cpp", "agg_shape_tests.cpp"), os.path.join(CSRC, "agg_shape.cpp")]
FLAGS = ["-std=c++17", "-O0", "-g", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + os.path.join(ROOT, "include"),
         "-I" + CSRC, "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections"]


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe] + SOURCES)
    needed = subprocess.run(["readelf", "-d", exe], capture_output=True, text=True, check=True).stdout
    assert "amdhip64" not in needed and "hiprtc" not in needed, needed
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout, r.stdout
    return r


def test_agg_shape_logic(tmp_path):
    _build_and_run(tmp_path, "agg_shape_tests", [])


def test_agg_shape_logic_under_sanitizers(tmp_path):
    r = _build_and_run(tmp_path, "agg_shape_tests_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
