"""CPU: the sparse crossover's host set-up (smart-crossover_amd/csrc/sx_band_plan.h) under the host sanitizers.

tests/native/band_plan_check.cpp -- a program of its own that includes nothing but the plan -- is compiled with the
host compiler, AddressSanitizer and UBSan, and run once per case on small LPs written to raw files.  It walks the
stages in the driver's order and checks what they promise each other (one variable per band position, a column only
on a row it has an entry in, eqidx one-to-one, padding as unit columns, no triplet across blocks or outside kl / ku,
a border of exactly ndr + h columns, m basic variables and none twice, ...); the first violated invariant is printed
and the exit status is 1.  Nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import workloads

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
    exe = tmp_path_factory.mktemp("band_plan") / "band_plan_check"
    cmd = [CXX, *FLAGS, *link_flags(), "-I", os.path.join(ROOT, "smart-crossover_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "band_plan_check.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(case_dir, *args):
        got = subprocess.run([str(exe), str(case_dir), *args], capture_output=True, text=True)
        assert got.returncode == 0, f"{' '.join(args)}\n{got.stdout}\n{got.stderr}"
        assert got.stdout.rstrip().endswith("OK")
        return got.stdout
    return run


def write_lp(path, A, b, l, u, lt, x):
    """CSC, CSR, bounds, the point and its slacks b - A x as raw little-endian arrays."""
    path.mkdir()
    csr = sp.csr_matrix(A)
    csr.sort_indices()
    csc = csr.tocsc()
    csc.sort_indices()
    for name, arr, dt in [("cptr.i64", csc.indptr, np.int64), ("cidx.i32", csc.indices, np.int32), ("cval.f64", csc.data, np.float64),
                          ("rptr.i64", csr.indptr, np.int64), ("ridx.i32", csr.indices, np.int32), ("lo.f64", l, np.float64),
                          ("up.f64", u, np.float64), ("b.f64", b, np.float64), ("lt.u8", lt, np.uint8), ("x.f64", x, np.float64),
                          ("slack.f64", b - csr @ x, np.float64)]:
        np.ascontiguousarray(arr, dtype=dt).tofile(path / name)
    return path


def write_instance(path, inst, rows=None, cols=None):
    A = inst.A
    b, l, u, lt, x = inst.b, inst.l, inst.u, inst.sense == "<", inst.x
    if rows is not None:
        A, b, lt = A[rows], b[rows], lt[rows]
    if cols is not None:
        A, l, u, x = A[:, cols], l[cols], u[cols], x[cols]
    return write_lp(path, A, b, l, u, lt, x)


@pytest.fixture(scope="module")
def staircase(tmp_path_factory):
    """netlib_lp(800, 8000): 8 linking rows of ~1,000 entries over a dense threshold of 480."""
    return write_instance(tmp_path_factory.mktemp("lp") / "staircase", workloads.netlib_lp(800, 8000))


def test_natural_staircase_guessed_basis_one_block(check, staircase):
    check(staircase, "expect_P=1")


# A cut into P blocks is taken only when rl >= 4 * pad, pad = roundup(kl + ku + 32, 32), rl = the block length rounded down
# to 32.  This generator's matched band has kl and ku of 111 .. 119 each at these sizes (window 48: a column reaches up
# to 96 rows ahead of its own row, and an own row may hold a column from 24 rows away), so pad = 288 and a block needs
# 1,152 positions beside separators of ~118: 800 rows admit no cut (checked below).  Two blocks need 2 * 1152 + 118 =
# 2,422 band rows, three 3 * 1152 + 2 * 118 = 3,692; 1 % of the rows are linking rows.  In steps of 100 rows these are the
# smallest that admit the cut: the test shows that 100 rows fewer get one block less.
BLOCK_CASES = [(2, 2500), (3, 3800)]


@pytest.mark.parametrize("blocks,m", BLOCK_CASES)
def test_blocks_cut_at_separators(check, tmp_path, blocks, m):
    d = write_instance(tmp_path / "lp", workloads.netlib_lp(m, 10 * m))
    check(d, f"blocks={blocks}", f"expect_P={blocks}")
    # the synthetic LU outcomes on a cut band as well: replaced columns and row swaps within blocks, both repair branches
    check(d, f"blocks={blocks}", f"expect_P={blocks}", "lu=synthetic", "schur=synthetic")
    smaller = write_instance(tmp_path / "smaller", workloads.netlib_lp(m - 100, 10 * (m - 100)))
    check(smaller, f"blocks={blocks}", f"expect_P={blocks - 1}")


def test_too_small_for_the_requested_blocks_takes_fewer(check, staircase):
    check(staircase, "blocks=3", "expect_P=1")


def test_shuffled_rows_fall_back_into_stages(check, tmp_path):
    """Rows and columns permuted, m just large enough that the tallest column passes the 600-row trigger of the
    Cuthill-McKee order: that order must not be taller than the natural one, and the plan must take it."""
    inst = workloads.netlib_lp(1500, 15000)
    rng = np.random.default_rng(5)
    d = write_instance(tmp_path / "lp", inst, rows=rng.permutation(1500), cols=rng.permutation(15000))
    check(d, "expect_cm=1")


def test_given_basis_with_columns_at_upper_and_superbasic(check, staircase, tmp_path):
    staircase = shutil.copytree(staircase, tmp_path / "lp")     # (the program writes the basis beside the LP)
    check(staircase, "write_basis=1")
    vb = np.fromfile(staircase / "vb.i8", dtype=np.int8)
    u = np.fromfile(staircase / "up.f64", dtype=np.float64)
    nonbasic = np.flatnonzero(vb != 0)
    vb[nonbasic[::7]] = -2          # (finite and infinite upper bounds both: the latter rest at the lower bound)
    vb[nonbasic[3::11]] = -3
    assert np.isinf(u[vb == -2]).any() and np.isfinite(u[vb == -2]).any() and (vb == -3).sum() > 100
    vb.tofile(staircase / "vb.i8")
    check(staircase, "basis=given")
    check(staircase, "basis=given", "lu=synthetic", "schur=synthetic")


def test_synthetic_band_lu_outcome_and_both_repairs_of_the_dense_lu(check, staircase):
    out = check(staircase, "lu=synthetic", "schur=synthetic")
    assert "band LU: 8 columns replaced" in out


@pytest.mark.parametrize("perturb,branch", [("few", "placeholders became logicals"), ("slack", "logicals of border rows filled in"),
                                            ("many", "columns went superbasic")])
def test_border_with_too_few_and_too_many_columns(check, staircase, perturb, branch):
    """A basic set short of columns (every tenth and the dense rows' own), the band rows' logicals alone, and one with
    columns to spare: each must balance through its own branch -- placeholders turn into their rows' logicals, the dense
    rows' logicals fill in, the surplus goes superbasic -- and the program's count of that branch must not be 0."""
    out = check(staircase, f"perturb={perturb}", "lu=synthetic")
    counts = re.search(r"balancing: (\d+) placeholders became logicals, (\d+) logicals of border rows filled in, (\d+) columns went superbasic", out)
    taken = dict(zip(["placeholders became logicals", "logicals of border rows filled in", "columns went superbasic"], map(int, counts.groups())))
    assert taken[branch] > 0, out


def test_one_dense_row_goes_to_the_border(check, tmp_path):
    """netlib_lp(150, 1500) has ONE linking row (1,500 entries, threshold 480)."""
    out = check(write_instance(tmp_path / "lp", workloads.netlib_lp(150, 1500)))
    assert "149 band rows, 1 dense" in out and "(1 dense or separator" in out


def test_hand_written_case_pins_the_greedy_order(check, tmp_path):
    """Six rows, eight columns, a given basis {c0 .. c5}; expected values derived by hand from the rule "size descending,
    then variable, then row", two rounds (first every column's largest eligible entry, then all entries of the losers).

        row   c0    c1    c2    c3     c4    c5    c6   c7
         0    2.0   3.0                      0.1
         1    1.0         1.0                0.1
         2    1.0   0.5   1.0
         3    1.0               1e-7   0.25
         4                      0.5    0.5
         5                                         1.0  1.0

    Round 1 (one candidate per column; within a column ties go to the smaller row; 1e-7 is below the 1e-6 a column may
    sit on): c1 (3.0, r0), c0 (2.0, r0), c2 (1.0, r1), c3 (0.5, r4), c4 (0.5, r4), c5 (0.1, r0).  In that order: c1 takes
    r0, c0 loses, c2 takes r1, c3 takes r4 (before c4: equal size, smaller variable), c4 and c5 lose.
    Round 2 (all entries of the losers in rows still free): c0 (1.0, r2), c0 (1.0, r3), c4 (0.25, r3); c5 has none.
    c0 takes r2 -- equal sizes of one column go by row; by descending row c0 would take r3 and c4 find nothing --, c4 takes
    r3.  Row 5 stays a placeholder, c5 goes to the border: head = band positions, then the border column.
    Widths: position 0 holds c1 (rows 0, 2): kl = 2; position 2 holds c0 (rows 0 .. 3): ku = 2."""
    rows = [0, 1, 2, 3, 0, 2, 1, 2, 3, 4, 4, 3, 0, 1, 5, 5]
    cols = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7]
    vals = [2.0, 1.0, 1.0, 1.0, 3.0, 0.5, 1.0, 1.0, 1e-7, 0.5, 0.5, 0.25, 0.1, 0.1, 1.0, 1.0]
    A = sp.coo_matrix((vals, (rows, cols)), shape=(6, 8))
    l, u = np.zeros(8), np.array([np.inf] * 6 + [4.0, np.inf])
    x = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.5])
    d = write_lp(tmp_path / "lp", A, A @ x, l, u, np.zeros(6, dtype=np.uint8), x)
    np.array([0, 0, 0, 0, 0, 0, -2, -3], dtype=np.int8).tofile(d / "vb.i8")
    np.full(6, -1, dtype=np.int8).tofile(d / "cb.i8")
    (d / "expect.txt").write_text(
        "matching 1 2 0 4 3 -1\n"
        "geometry 1 6 0 0 6 6 6 0 2 2\n"      # P RL Wsep PAD stride RL_last m1 ndr kl ku
        "eqidx 0 1 2 3 4 5\n"
        "head 1 2 0 4 3 -1 5\n"
        "varJ 7\n")
    check(d, "basis=given", f"expect={d / 'expect.txt'}")
