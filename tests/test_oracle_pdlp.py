"""CPU: oracle/pdlp.py (the statement of the first-order stage K16p) reaches HiGHS' optimal value and a
primal-dual pair that satisfies the LP's optimality conditions.  The reference runs Gurobi's barrier at this
point (lp_methods/algorithms.py:50-54): parity unpinned, HiGHS stands in as the independent solver.  The inputs
with general bounds, long rows and empty segments (tests/_pdlp_cases.py) are checked here before the device is
held to the oracle at them (tests/test_gpu_pdlp_edges.py)."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import pdlp as P
import workloads

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _pdlp_cases as PC  # noqa: E402

highs = PC.highs


def reaches_the_optimum(inst):
    out = P.pdlp(inst.A, inst.b, inst.c, inst.l, inst.u, inst.sense == "<", inst.x, inst.y, max_iter=200000, tol=1e-9)
    ref = highs(inst)
    assert out["status"] == 0
    assert out["primal_obj"] == pytest.approx(ref.fun, rel=1e-6, abs=1e-6)
    x, y = out["x"], out["y"]
    lt = inst.sense == "<"
    r = inst.b - inst.A @ x
    assert np.abs(r[~lt]).max(initial=0) < 1e-6 and r[lt].min(initial=0) > -1e-6
    assert np.all(x >= inst.l) and np.all(x <= inst.u) and np.all(y[lt] <= 0)
    return ref


@pytest.mark.parametrize("m,n,k,seed", [(27, 51, 2, 2024), (60, 200, 4, 1), (150, 400, 5, 2)])
def test_oracle_pdlp_reaches_the_optimum(m, n, k, seed):
    inst = workloads.sparse_lp(m, n, k, seed=seed, stratified=False)
    # the crossover's situation: an interior point of the LP, a perturbed cost (lp_methods/algorithms.py:148-151)
    inst.c = inst.c + 1e-2 * np.random.default_rng(seed).uniform(0.9, 1.0, n) / np.maximum(inst.x, 1e-6).clip(1e-2)
    reaches_the_optimum(inst)


@pytest.mark.parametrize("m,n,k,seed,free,uponly,fun", [(150, 400, 5, 2, 40, 14, -255.19659), (60, 200, 4, 1, 19, 13, None)])
def test_oracle_pdlp_reaches_the_optimum_at_general_bounds(m, n, k, seed, free, uponly, fun):
    """Free columns, columns bounded only above, boxes shifted to negative / non-zero lower bounds."""
    inst = PC.general_bounds_lp(m, n, k, seed)
    no_l, no_u = np.isinf(inst.l), np.isinf(inst.u)
    assert np.count_nonzero(no_l & no_u) == free and np.count_nonzero(no_l & ~no_u) == uponly
    assert np.count_nonzero(~no_l & (inst.l < 0)) > 0 and np.count_nonzero(~no_l & (inst.l > 0)) > 0
    ref = reaches_the_optimum(inst)
    if fun is not None:
        assert ref.fun == pytest.approx(fun, abs=1e-5)          # (the instance the recorded figures belong to)


def test_oracle_pdlp_reduced_costs_of_both_signs_on_every_kind_of_column():
    """What the general-bounds case exists for: after 256 cold iterations c - A^T y is positive on columns without a
    lower bound, negative on columns without an upper bound (the dual residual) and of both signs on boxes with
    finite non-zero bounds (the bound term of the dual objective)."""
    inst = PC.general_bounds_lp(150, 400, 5, 2)
    out = P.pdlp(inst.A, inst.b, inst.c, inst.l, inst.u, inst.sense == "<", None, None, max_iter=256, tol=1e-14)
    assert out["restarts"] == 3
    rc = inst.c - inst.A.T @ out["y"]
    box = np.isfinite(inst.l) & np.isfinite(inst.u) & (inst.l != 0)
    assert np.count_nonzero((rc > 0) & np.isinf(inst.l)) == 16 and np.count_nonzero((rc < 0) & np.isinf(inst.u)) == 55
    assert np.any((rc > 0) & box) and np.any((rc < 0) & box)
    want = PC.record(inst.A, inst.b, inst.c, inst.l, inst.u, inst.sense == "<", out["x"], out["y"])
    assert want["dual_residual"] > 1e-3
    for key in ("primal_obj", "dual_obj", "gap"):
        assert out[key] == pytest.approx(want[key], rel=1e-9, abs=1e-9)
    for key in ("primal_residual", "dual_residual"):
        assert out[key] == pytest.approx(want[key], rel=1e-6, abs=1e-12)


def test_oracle_pdlp_long_rows_and_empty_segments():
    """Rows and a column longer than a chunk of the device's walks, empty rows and empty columns: the structure, and 256
    iterations that stay finite (the scalings leave an empty segment's scale alone) with the empty columns at the bound
    their cost pushes them to.  (To HiGHS' optimum, -836.77195, the oracle needs 232,000 iterations: too long here.)"""
    inst = PC.long_rows_lp(1300, 2600, 3, seed=12)
    PC.check_long_rows(inst)
    dr, dc = P.scalings(inst.A)
    rows, cols = PC.segment_lengths(inst.A)
    assert np.all(dr[rows == 0] == 1.0) and np.all(dc[cols == 0] == 1.0) and np.all(np.isfinite(dr)) and np.all(np.isfinite(dc))
    out = P.pdlp(inst.A, inst.b, inst.c, inst.l, inst.u, inst.sense == "<", inst.x, inst.y, max_iter=256, tol=1e-14)
    assert out["iters"] == 256 and out["status"] == 3
    assert np.all(np.isfinite(out["x"])) and np.all(np.isfinite(out["y"]))
    assert all(np.isfinite(out[k]) for k in ("primal_residual", "dual_residual", "gap", "primal_obj", "dual_obj", "primal_weight"))
    assert out["x"][5] == 0.0 and out["x"][6] == 2.0
    want = PC.record(inst.A, inst.b, inst.c, inst.l, inst.u, inst.sense == "<", out["x"], out["y"])
    for key in ("primal_obj", "dual_obj", "gap"):
        assert out[key] == pytest.approx(want[key], rel=1e-9, abs=1e-9)


def test_kkt_by_hand_one_column_of_each_bound_type():
    """A = [1 2 0 -1; 0 1 3 1], row 0 '=', row 1 '<'; columns [0, inf), (-inf, 3], (-inf, inf), [-2, 5];
    x = (1, 2, -1, 0.5), y = (1, -2), b = (4, 1).
      A x = (4.5, -0.5): b - A x = (-0.5, 1.5), the '<' row is satisfied            -> pr = 0.5
      A^T y = (1, 0, -6, -3), b^T y = 2
    first cost c = (3, 0.5, -7.5, -2):  rc = (2, 0.5, -1.5, 1)
      column 0: rc > 0, l = 0     -> bound 0         column 1: rc > 0, l = -inf -> violation 0.5
      column 2: rc < 0, u = inf   -> violation -1.5  column 3: rc > 0, l = -2   -> bound -2
      du = sqrt(0.25 + 2.25), dobj = 2 - 2 = 0, pobj = 3 + 1 + 7.5 - 1 = 10.5, gap = 10.5
    second cost c = (-1, -0.5, -4.5, -4):  rc = (-2, -0.5, 1.5, -1)
      column 0: rc < 0, u = inf   -> violation -2    column 1: rc < 0, u = 3    -> bound -1.5
      column 2: rc > 0, l = -inf  -> violation 1.5   column 3: rc < 0, u = 5    -> bound -5
      du = sqrt(4 + 2.25) = 2.5, dobj = 2 - 6.5 = -4.5, pobj = -1 - 1 + 4.5 - 2 = 0.5, gap = 5"""
    A = sp.csr_matrix(np.array([[1.0, 2.0, 0.0, -1.0], [0.0, 1.0, 3.0, 1.0]]))
    AT = A.T.tocsr()
    b, lt = np.array([4.0, 1.0]), np.array([False, True])
    l, u = np.array([0.0, -np.inf, -np.inf, -2.0]), np.array([np.inf, 3.0, np.inf, 5.0])
    x, y = np.array([1.0, 2.0, -1.0, 0.5]), np.array([1.0, -2.0])
    for c, du, dobj, pobj, gap in ((np.array([3.0, 0.5, -7.5, -2.0]), np.sqrt(2.5), 0.0, 10.5, 10.5),
                                   (np.array([-1.0, -0.5, -4.5, -4.0]), 2.5, -4.5, 0.5, 5.0)):
        k = P.kkt(A, AT, b, c, l, u, lt, x, y)
        assert k["pr"] == 0.5 and k["pobj"] == pobj and k["dobj"] == dobj and k["gap"] == gap
        assert k["du"] == pytest.approx(du, rel=1e-15)
        assert k["err"] == pytest.approx(np.sqrt(0.25 + du * du + gap * gap), rel=1e-15)
        assert k["rcnorm"] == pytest.approx(np.sqrt(4 + 0.25 + 2.25 + 1), rel=1e-15)
        got = PC.record(A, b, c, l, u, lt, x, y)                # the tests' own statement of the record agrees
        assert (got["primal_residual"], got["primal_obj"], got["dual_obj"], got["gap"]) == (0.5, pobj, dobj, gap)
        assert got["dual_residual"] == pytest.approx(du, rel=1e-15)
    # a violated '<' row counts, a violated '=' row counts with either sign
    k = P.kkt(A, AT, np.array([5.0, -1.0]), c, l, u, lt, x, y)   # b - A x = (0.5, -0.5)
    assert k["pr"] == pytest.approx(np.sqrt(0.5), rel=1e-15)


def test_oracle_pdlp_iteration_limit_and_cold_start():
    inst = workloads.sparse_lp(40, 120, 3, seed=5, stratified=False)
    out = P.pdlp(inst.A, inst.b, inst.c, inst.l, inst.u, inst.sense == "<", None, None, max_iter=100, tol=1e-12)
    assert out["status"] == 3 and out["iters"] == 128          # rounded up to whole periods of 64
    dr, dc = P.scalings(inst.A)
    assert P.operator_norm(inst.A, dr, dc) <= 1.0 + 1e-12       # Pock-Chambolle (alpha = 1) bounds the norm by 1
