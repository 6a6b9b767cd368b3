"""The scoring plan (nanomotif_amd/csrc/nmscore_plan.h) against the restatement of tools/plan_check/driver.cpp, on the CPU: validation,
stable sort, ranges, staging layout, own segment table, light / heavy and compile crossovers, and the grid's cover of every chunk.
The driver is an executable of its own; where the address and undefined-behaviour sanitizers link it runs a second time under them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tools", "plan_check", "driver.cpp")
CXX = os.environ.get("CXX", "g++")


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    return exe, subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", *flags, DRIVER, "-o", exe], capture_output=True, text=True)


def _run(exe, *args):
    done = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "plan_check ok" in done.stdout
    return done.stdout


@pytest.mark.skipif(shutil.which(CXX) is None, reason="no host C++ compiler")
def test_plan_matches_its_restatement(tmp_path):
    exe, built = _build(tmp_path, "plan_check", ["-O2"])
    assert built.returncode == 0, built.stderr
    print(_run(exe))
    print(_run(exe, "77", "1500"))                      # another seed


@pytest.mark.skipif(shutil.which(CXX) is None, reason="no host C++ compiler")
def test_plan_under_address_and_undefined_sanitizers(tmp_path):
    exe, built = _build(tmp_path, "plan_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr):
        pytest.skip("the sanitizer runtimes do not link here")
    assert built.returncode == 0, built.stderr
    print(_run(exe, "20240521", "1200"))
