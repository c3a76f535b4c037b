"""CPU: the host arithmetic of the projector CG (smart-crossover_amd/csrc/sx_cg_plan.h) under the host sanitizers.

tests/native/cg_plan_check.cpp -- a program of its own that includes nothing but the plan -- is compiled with the host
compiler, AddressSanitizer and UBSan, and run once per group of cases: the walk grid and the vector grid at the sizes
where their clamps and roundings step, the workspace layout against the formula the drivers used before the plan existed,
and the two stopping rules side by side, including the one case (tol > 1) in which they differ on purpose.  The first
violated expectation is printed and the exit status is 1.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wshadow", "-Werror", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined"]

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler on PATH")


def link_flags():
    """g++ links the sanitizers' runtimes as shared libraries, which refuse to start when another library is preloaded in
    front of them; linked statically (clang++'s default) the program starts in whatever environment the suite runs in,
    which is passed on untouched."""
    version = subprocess.run([CXX, "--version"], capture_output=True, text=True).stdout
    return ["-static-libasan", "-static-libubsan"] if "Free Software Foundation" in version else []


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cg_plan") / "cg_plan_check"
    cmd = [CXX, *FLAGS, *link_flags(), "-I", os.path.join(ROOT, "smart-crossover_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "cg_plan_check.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(case):
        got = subprocess.run([str(exe), case], capture_output=True, text=True)
        assert got.returncode == 0, f"{case}\n{got.stdout}\n{got.stderr}"
        assert got.stdout.rstrip().endswith("OK")
    return run


def test_walk_grid(check):
    """0, 1, 63, 64, 65, 2047, 2048, 2049 and 5000 tiles, with the XCD map on and off."""
    check("walk_grid")


def test_vector_grid(check):
    """Lengths 0, 1, 4 WG, 4 WG + 1, 1024 * 4 WG and one above."""
    check("vector_grid")


def test_layout_regions_and_bytes(check):
    """(m, n) in (1, 0), (1, 1), (7, 3), (1000, 5000): aligned, disjoint, inside `bytes`, and `bytes` is the formula that
    the single-device and the sharded driver each had of their own."""
    check("layout")


def test_stopping_rules_single_and_sharded(check):
    """||b|| = 0, = tol, just above tol, and tol = 2 -- where the single-device rule skips the loop without `done` and the
    sharded rule sets it."""
    check("stopping")
