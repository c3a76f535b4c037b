"""General column bounds made from the LPs the suite already trusts (workloads.netlib_lp and friends draw l = 0 with
u = inf or a positive finite u only).  Used by tests/test_general_bounds_cpu.py (pinned against HiGHS alone),
tests/test_gpu_crossover_band_bounds.py (K16s) and tests/_dist_worker4.py (ShardedLP.restricted_resolve).

  affine_image  the same LP under x = d * x' + t, d = +-1 per column: upper-only columns, negative and non-zero
                lower bounds, boxes that straddle 0, interior points far from 0 -- same pattern, same conditioning,
                same (unique) optimum up to the constant c @ t;
  fix_some      l = u at the value of chosen columns;
  free_some     l = -inf, u = inf on chosen columns.

The order of the random draws is part of the cases.  Plain numpy / scipy, no dependency on the product package.
"""
import dataclasses

import numpy as np
import scipy.sparse as sp
from scipy.optimize import linprog

KEEP, SHIFT, MIRROR, MIRROR_SHIFT = 0, 1, 2, 3


def affine_image(inst, seed):
    """(image, d, t, const): `inst` under x = d * x' + t.  A kind per column, uniform over {keep, shift, mirror,
    mirror + shift}; d = -1 for the two mirror kinds, t ~ U(-5, 5) for the two shift kinds.  The image's optimal value
    plus const = c @ t is the original's; x' = d * (x - t), y' = y."""
    rng = np.random.default_rng(seed)
    n = inst.c.size
    kind = rng.integers(0, 4, n)
    d = np.where((kind == MIRROR) | (kind == MIRROR_SHIFT), -1.0, 1.0)
    t = np.where((kind == SHIFT) | (kind == MIRROR_SHIFT), rng.uniform(-5.0, 5.0, n), 0.0)
    A = sp.csr_matrix(inst.A)
    A2 = sp.csr_matrix(A @ sp.diags(d))
    A2.sort_indices()
    lo = np.where(d > 0, inst.l - t, t - inst.u)
    up = np.where(d > 0, inst.u - t, t - inst.l)
    image = dataclasses.replace(inst, A=A2, b=inst.b - A @ t, c=d * inst.c, l=lo, u=up, x=map_vertex(inst.x, d, t),
                                y=inst.y.copy())
    return image, d, t, float(inst.c @ t)


def map_vertex(x, d, t):
    return d * (np.asarray(x, dtype=np.float64) - t)


def map_basis(vbasis, d):
    """Column codes of the image: a mirrored column swaps -1 (at lower) and -2 (at upper)."""
    vb = np.asarray(vbasis).copy()
    mir = d < 0
    vb[mir & (np.asarray(vbasis) == -1)] = -2
    vb[mir & (np.asarray(vbasis) == -2)] = -1
    return vb


def fix_some(inst, cols, x_opt):
    """l = u = x_opt on `cols` (the caller picks non-basic columns that sit at a non-zero bound)."""
    cols = np.asarray(cols)
    l, u = inst.l.copy(), inst.u.copy()
    l[cols] = x_opt[cols]
    u[cols] = x_opt[cols]
    return dataclasses.replace(inst, l=l, u=u)


def free_some(inst, cols):
    cols = np.asarray(cols)
    l, u = inst.l.copy(), inst.u.copy()
    l[cols], u[cols] = -np.inf, np.inf
    return dataclasses.replace(inst, l=l, u=u)


def column_kinds(inst):
    """Counts of lower-only, upper-only, boxed and free columns, and of finite lower bounds that are not 0."""
    fl, fu = np.isfinite(inst.l), np.isfinite(inst.u)
    return {"lower_only": int(np.count_nonzero(fl & ~fu)), "upper_only": int(np.count_nonzero(~fl & fu)),
            "boxed": int(np.count_nonzero(fl & fu)), "free": int(np.count_nonzero(~fl & ~fu)),
            "nonzero_lower": int(np.count_nonzero(fl & (inst.l != 0.0)))}


def highs(inst, c=None):
    """HiGHS on the instance, unchecked: the caller reads .status (0 optimal, 2 infeasible, 3 unbounded)."""
    lt = np.asarray(inst.sense) == "<"
    fin = lambda v: [None if np.isinf(s) else float(s) for s in v]   # noqa: E731
    return linprog(inst.c if c is None else c, A_ub=inst.A[lt], b_ub=inst.b[lt], A_eq=inst.A[~lt], b_eq=inst.b[~lt],
                   bounds=list(zip(fin(inst.l), fin(inst.u))), method="highs")


def basis_of(inst, x, tol=1e-7):
    """Codes of a non-degenerate vertex read off the point: -1 at lower, -2 at upper, 0 in between."""
    vb = np.zeros(x.size, dtype=np.int8)
    vb[np.abs(x - inst.l) <= tol] = -1
    vb[np.abs(inst.u - x) <= tol] = -2
    return vb
