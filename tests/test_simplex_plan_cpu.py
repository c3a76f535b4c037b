"""CPU: the host arithmetic of the dense simplex driver (smart-crossover_amd/csrc/sx_simplex_plan.h) under the host
sanitizers.

tests/native/simplex_plan_check.cpp -- a program of its own that includes nothing but the plan -- is compiled with the
host compiler, AddressSanitizer and UBSan, and run once per group of cases: the kept-inverse test on hand-written heads
(every way a head can fail to belong to the basis handed in), the round trip head -> ids -> head under shuffled columns,
the refresh interval against its formula, the arena size against a replay of the driver's requests, the fold grids and
the status ladders.  The first violated expectation is printed and the exit status is 1.  Nothing is loaded into Python."""
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
    exe = tmp_path_factory.mktemp("simplex_plan") / "simplex_plan_check"
    cmd = [CXX, *FLAGS, *link_flags(), "-I", os.path.join(ROOT, "smart-crossover_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "simplex_plan_check.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(case):
        got = subprocess.run([str(exe), case], capture_output=True, text=True)
        assert got.returncode == 0, f"{case}\n{got.stdout}\n{got.stderr}"
        assert got.stdout.rstrip().endswith("OK")
    return run


def test_kept_head_belongs_to_the_basis_handed_in_or_is_refused(check):
    """Accepted under a permutation of the columns; refused with a basic column missing, extra or left over, two columns
    of one id, a logical whose row went non-basic or lies at row m, head_ids of the wrong length; m = 1 and n = 0."""
    check("kept_head")


def test_head_ids_round_trip_under_shuffled_columns(check):
    check("round_trip")


def test_refresh_interval_follows_its_formula(check):
    """m = 1, 2047, 2048, 2896, 11585 and 10^6 (and the neighbours at which the rounded value steps)."""
    check("refresh")


def test_arena_holds_every_request_of_the_driver(check):
    """m in {1, 63, 64, 1000}, with and without deferred updates, Devex weights and a session."""
    check("arena")


def test_fold_grids(check):
    """m = 1, 15, 16, 255, 256, 257 (and two sizes past one super-block of the matrix-core fold)."""
    check("fold")


def test_limits_and_status_ladders(check):
    check("misc")
