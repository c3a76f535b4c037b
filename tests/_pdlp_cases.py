"""Inputs of the first-order stage's tests (K16p: tests/test_oracle_pdlp.py on the CPU, tests/test_gpu_pdlp_edges.py on
the device) beyond what workloads.sparse_lp gives, which is l = 0 everywhere and at most a dozen entries per row:

  general_bounds  free columns, columns bounded only above, boxes shifted to negative / non-zero finite bounds;
  long_rows_lp    a '<' and an '=' linking row and a column longer than one chunk of the walks (1,024 entries),
                  two empty rows and two empty columns;
  many_tiles_lp   more than 256 row tiles and more than 256 column tiles (a tile holds at most 256 segments).

The order of the random draws is part of the cases: recorded figures (restart counts, HiGHS' optimal values) depend on it.
Plain numpy / scipy, no dependency on the product package.
"""
import numpy as np
import scipy.sparse as sp
from scipy.optimize import linprog

import workloads

CHUNK = 1024      # PD_CHUNK of csrc/sx_pdlp.hip: entries staged per chunk of a walk
TILE = 256        # SX_WG of csrc/sx_segwalk.h: most segments in one tile


def perturb(inst, seed):
    """The perturbed cost of the crossover's sub-problem (lp_methods/algorithms.py:148-151), as in test_gpu_pdlp.py."""
    n = inst.c.size
    inst.c = inst.c + 1e-2 * np.random.default_rng(seed).uniform(0.9, 1.0, n) / np.maximum(inst.x, 1e-2)


def general_bounds(inst, seed):
    """Shift half of the boxes, free a share of the basic columns, drop the lower bound of half of the columns at
    their upper bound; (x, y) keeps its interior-point shape.  Call BEFORE perturb."""
    rng = np.random.default_rng(seed + 1000)
    n = inst.c.size
    l, u, x = inst.l.copy(), inst.u.copy(), inst.x.copy()
    basic = (x > 1e-3) & (x < u - 1e-3)
    at_up = np.isfinite(u) & (x > u - 1e-3)
    d = np.where(rng.random(n) < 0.5, rng.uniform(-3, 3, n), 0.0)     # shifted boxes: negative / non-zero finite l
    x, l, u = x + d, l + d, u + d
    b = inst.b + inst.A @ d
    free = basic & (rng.random(n) < 0.3)
    l[free], u[free] = -np.inf, np.inf
    uponly = at_up & (rng.random(n) < 0.5)
    l[uponly] = -np.inf                                               # bounded above only
    inst.l, inst.u, inst.x, inst.b = l, u, x, b


def general_bounds_lp(m, n, k, seed):
    """Case A."""
    inst = workloads.sparse_lp(m, n, k, seed=seed, stratified=False)
    general_bounds(inst, seed)
    perturb(inst, seed)
    return inst


def long_rows_lp(m, n, k, seed):
    """Case B."""
    inst = workloads.sparse_lp(m, n, k, seed=seed, stratified=False)
    rng = np.random.default_rng(seed + 500)
    A = sp.lil_matrix(inst.A)
    lt = inst.sense == "<"
    r_lt, r_eq = int(np.flatnonzero(lt)[3]), int(np.flatnonzero(~lt)[5])
    for r, cnt in ((r_lt, 1500), (r_eq, 2500)):                        # a '<' and an '=' linking row
        cols = rng.choice(n, cnt, replace=False)
        A[r, cols] = rng.uniform(-1, 1, cnt)
    rows = rng.choice(m, 1200, replace=False)
    A[rows, 77] = rng.uniform(-1, 1, 1200)                             # a long column
    e_eq, e_lt = int(np.flatnonzero(~lt)[9]), int(np.flatnonzero(lt)[9])
    A[e_eq, :] = 0
    A[e_lt, :] = 0
    A[:, 5] = 0
    A[:, 6] = 0                                                        # two empty rows, two empty columns
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    A.sort_indices()
    x, y, u = inst.x, inst.y, inst.u
    s_d = inst.c - inst.A.T @ y
    c = A.T @ y + s_d
    c[5] = 0.7
    u[6] = 2.0
    c[6] = -0.4
    x[5] = 0.0
    x[6] = 2.0                                                         # empty columns: one goes to l = 0, one to a finite u
    slack = inst.b - inst.A @ x
    b = A @ x + slack
    b[e_eq] = 0.0
    b[e_lt] = 0.5
    y[e_eq] = 0.3
    y[e_lt] = 0.0
    inst.A, inst.b, inst.c = A, b, c
    perturb(inst, seed)
    return inst


def many_tiles_lp():
    """Case C."""
    inst = workloads.sparse_lp(66000, 70000, 3, seed=4, stratified=True)
    perturb(inst, 4)
    return inst


def segment_lengths(A):
    """(entries per row, entries per column)."""
    A = sp.csr_matrix(A)
    return np.diff(A.indptr), np.diff(A.tocsc().indptr)


def check_long_rows(inst):
    """What case B exists for, asserted on the input itself."""
    rows, cols = segment_lengths(inst.A)
    lt = inst.sense == "<"
    long_rows = np.flatnonzero(rows > CHUNK)
    assert long_rows.size == 2 and np.count_nonzero(lt[long_rows]) == 1      # one '<', one '='
    assert np.count_nonzero(cols > CHUNK) == 1
    empty = np.flatnonzero(rows == 0)
    assert empty.size == 2 and np.count_nonzero(lt[empty]) == 1
    assert np.array_equal(np.flatnonzero(cols == 0), [5, 6])
    assert inst.l[5] == 0.0 and inst.c[5] > 0 and inst.u[6] == 2.0 and inst.c[6] < 0


def check_many_tiles(inst):
    m, n = inst.A.shape
    assert -(-m // TILE) > 256 and -(-n // TILE) > 256


def highs(inst):
    """HiGHS on the instance: the independent solver.  None stands for an infinite bound on either side."""
    lt = inst.sense == "<"
    fin = lambda v: [None if np.isinf(t) else float(t) for t in v]   # noqa: E731
    r = linprog(inst.c, A_ub=inst.A[lt], b_ub=inst.b[lt], A_eq=inst.A[~lt], b_eq=inst.b[~lt],
                bounds=list(zip(fin(inst.l), fin(inst.u))), method="highs")
    assert r.status == 0
    return r


def record(A, b, c, l, u, lt, x, y):
    """The record of include/sxhip.h (sx_pdlp_result) at the point (x, y), in np.longdouble, written from the
    header's statement and not from oracle/pdlp.py:
      primal_residual  || violation of A x (= | <=) b ||_2
      dual_residual    || part of rc = c - A^T y no bound can absorb ||_2: rc_j > 0 needs a finite l_j, rc_j < 0 a finite u_j
      dual_obj         b^T y + l^T rc+ + u^T rc-   (over the finite bounds)
      gap              | c^T x - dual_obj |"""
    L = np.longdouble
    A = sp.csr_matrix(A)
    m, n = A.shape
    xl, yl = np.asarray(x, dtype=L), np.asarray(y, dtype=L)
    val = A.data.astype(L)
    row = np.repeat(np.arange(m), np.diff(A.indptr))
    ax, aty = np.zeros(m, dtype=L), np.zeros(n, dtype=L)
    np.add.at(ax, row, val * xl[A.indices])
    np.add.at(aty, A.indices, val * yl[row])
    r = np.asarray(b, dtype=L) - ax
    r[lt] = np.minimum(r[lt], 0)
    rc = np.asarray(c, dtype=L) - aty
    pos, neg = rc > 0, rc < 0
    no_l, no_u = np.isinf(l), np.isinf(u)
    viol = np.where((pos & no_l) | (neg & no_u), rc, L(0))
    lf, uf = np.where(no_l, 0.0, l).astype(L), np.where(no_u, 0.0, u).astype(L)
    bound = np.where(pos & ~no_l, lf * rc, L(0)) + np.where(neg & ~no_u, uf * rc, L(0))
    pobj = np.asarray(c, dtype=L) @ xl
    dobj = np.asarray(b, dtype=L) @ yl + bound.sum()
    return {"primal_residual": float(np.sqrt(r @ r)), "dual_residual": float(np.sqrt(viol @ viol)),
            "primal_obj": float(pobj), "dual_obj": float(dobj), "gap": float(abs(pobj - dobj)), "rc": rc.astype(np.float64)}
