"""The wide JOIN key stage's per-row code without a GPU (csrc/device/qhip_widekey.inc: qh_wk_any_null, qh_wk_equal2, the build
row and the lookup row): tests/cpp/widekey_join_tests.cpp includes it as plain host C++, runs the build loop and then the lookup
loop single-threaded over small ragged tables whose buffers carry exactly the 64 bytes of slack every device allocation has, and
checks the build codes and the probe codes against a std::map of the keys without NULLs. Built with g++ as a stand-alone program
— nothing of it is loaded into Python — once plainly and once with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qurious_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "cpp", "widekey_join_tests.cpp")]
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + CSRC]


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe] + SOURCES)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout, r.stdout
    return r


def test_join_codes_match_a_map_of_the_keys(tmp_path):
    _build_and_run(tmp_path, "widekey_join_tests", [])


def test_join_codes_under_sanitizers(tmp_path):
    r = _build_and_run(tmp_path, "widekey_join_tests_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
