"""GPU: the first-order stage (K16p, csrc/sx_pdlp.hip) where tests/test_gpu_pdlp.py does not reach -- general bounds
(free columns, columns bounded only above, shifted boxes), rows and a column longer than one chunk of the walks, empty
rows and columns, more than 256 tiles per layout, every field of the result record, and the argument handling of
sx_pdlp_dev.  Inputs: tests/_pdlp_cases.py.  Yardsticks: oracle/pdlp.py step for step (the tolerances of
test_gpu_pdlp.py; the oracle against itself on a permuted copy of these inputs moves x and y by at most 1.3e-12 in the
same units and the gap by 3.3e-12 relative, profiles/r06/pdlp_edges.md), the record recomputed in np.longdouble from the
point handed back by the statement in include/sxhip.h, and HiGHS for the optimum.

Each comparison prints the share of its tolerance it used ("pdlp-edges ..." lines, shown with -s)."""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import pdlp as P
import workloads

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _pdlp_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LT = object()       # device(lt=LT): the mask of the instance


@pytest.fixture(scope="module")
def ctx():
    from smart_crossover.hip import default_context
    return default_context()


@functools.lru_cache(maxsize=None)
def case(name):
    """The instances, built once and never written to."""
    if name == "A150":
        return PC.general_bounds_lp(150, 400, 5, 2)
    if name == "A60":
        return PC.general_bounds_lp(60, 200, 4, 1)
    if name == "B":
        return PC.long_rows_lp(1500, 4000, 4, 11)
    if name == "C":
        return PC.many_tiles_lp()
    if name == "c1":
        inst = workloads.config1()
        PC.perturb(inst, 2024)
        return inst
    raise KeyError(name)


LONGER = {"A150": 256, "A60": 256, "B": 256, "C": 128}
# restarts of the oracle after 64 / the longer count of iterations (no decision closer than 1.3e-2 relative to its threshold)
RESTARTS = {("A150", True): (1, 2), ("A150", False): (1, 3), ("A60", True): (1, 3), ("A60", False): (1, 2),
            ("B", True): (1, 3), ("B", False): (1, 3), ("C", True): (1, 2)}


def device(ctx, inst, x0, y0, max_iter, tol, lt=LT, A=None):
    """test_gpu_pdlp.py's helper, with the row mask (None: the NULL pointer) and the matrix open to the caller."""
    m, n = inst.A.shape
    dA = ctx.matrix(inst.A) if A is None else A
    put = lambda v, t=np.float64: ctx.to_device(np.ascontiguousarray(v, dtype=t))   # noqa: E731
    d_x, d_y = ctx.empty(n, np.float64), ctx.empty(m, np.float64)
    mask = (inst.sense == "<") if lt is LT else lt
    try:
        res = ctx.pdlp(dA, put(inst.b), put(inst.c), put(inst.l), put(inst.u), None if mask is None else put(mask, np.uint8),
                       None if x0 is None else put(x0), None if y0 is None else put(y0), max_iter, tol, d_x, d_y)
        return res, d_x.download(), d_y.download()
    finally:
        if A is None:
            dA.free()


def oracle(inst, x0, y0, max_iter, tol=1e-14):
    return P.pdlp(inst.A, inst.b, inst.c, inst.l, inst.u, inst.sense == "<", x0, y0, max_iter=max_iter, tol=tol)


def used(got, want, rel, abs_=0.0):
    """Largest share of the tolerance max(abs_, rel |want|) that |got - want| takes; a NaN takes all of it."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.abs(got - want) / np.maximum(abs_, rel * np.abs(want))
    share = np.where(got == want, 0.0, share)
    return float(np.max(np.where(np.isnan(share), np.inf, share), initial=0.0))


# the tolerances of test_gpu_pdlp.py: field -> (rel, abs)
RECORD_TOL = {"primal_obj": (1e-9, 0.0), "dual_obj": (1e-9, 1e-9), "gap": (1e-9, 1e-9),
              "primal_residual": (1e-6, 1e-12), "dual_residual": (1e-6, 1e-12)}


def same_record(tag, res, want):
    shares = {k: used(getattr(res, k), want[k], *RECORD_TOL[k]) for k in RECORD_TOL}
    print(f"pdlp-edges {tag} record: " + " ".join(f"{k}={v:.3g}" for k, v in shares.items()))
    for k, (rel, abs_) in RECORD_TOL.items():
        assert float(getattr(res, k)) == pytest.approx(want[k], rel=rel, abs=abs_ if abs_ else None), k


def same_run(tag, res, x, y, want, iters):
    """Test 1's comparison of a device run with the oracle's."""
    assert int(res.status) == want["status"] == 3 and int(res.iters) == want["iters"] == iters
    print(f"pdlp-edges {tag} iters={iters} restarts={int(res.restarts)}/{want['restarts']} "
          f"x={used(x, want['x'], 1e-9, 1e-11):.3g} y={used(y, want['y'], 1e-9, 1e-11):.3g} "
          f"step={used(res.step, want['step'], 1e-10):.3g} primal_weight={used(res.primal_weight, want['primal_weight'], 1e-8):.3g}")
    assert int(res.restarts) == want["restarts"]
    assert float(res.step) == pytest.approx(want["step"], rel=1e-10)
    assert float(res.primal_weight) == pytest.approx(want["primal_weight"], rel=1e-8)
    np.testing.assert_allclose(x, want["x"], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(y, want["y"], rtol=1e-9, atol=1e-11)
    same_record(tag, res, want)


def forces_its_path(name, inst):
    """The property the case exists for, on the input itself."""
    if name in ("A150", "A60"):
        no_l, no_u = np.isinf(inst.l), np.isinf(inst.u)
        assert np.count_nonzero(no_l & no_u) == {"A150": 40, "A60": 19}[name]
        assert np.count_nonzero(no_l & ~no_u) == {"A150": 14, "A60": 13}[name]
        assert np.any(~no_l & (inst.l < 0)) and np.any(~no_l & (inst.l > 0))
    elif name == "B":
        PC.check_long_rows(inst)
    elif name == "C":
        PC.check_many_tiles(inst)


# ------------------------------------------------------------------------------------------ 1. step for step
@pytest.mark.parametrize("warm", [True, False], ids=["warm", "cold"])
@pytest.mark.parametrize("name", ["A150", "A60", "B", "C"])
def test_same_iteration_as_the_oracle(ctx, name, warm):
    inst = case(name)
    forces_its_path(name, inst)
    x0, y0 = (inst.x, inst.y) if warm else (None, None)
    for iters in (64, LONGER[name]):
        res, x, y = device(ctx, inst, x0, y0, iters, 1e-14)
        want = oracle(inst, x0, y0, iters)
        same_run(f"{name} {'warm' if warm else 'cold'}", res, x, y, want, iters)
        if (name, warm) in RESTARTS:
            assert want["restarts"] == RESTARTS[(name, warm)][0 if iters == 64 else 1]
    assert want["restarts"] >= 2        # a restart inside the run: the candidate of k_pd_apply became the iterate
    if name == "A150" and not warm:
        # reduced costs of both signs where a bound is missing (dual residual) and on shifted boxes (bound term)
        rc = inst.c - inst.A.T @ want["y"]
        box = np.isfinite(inst.l) & np.isfinite(inst.u) & (inst.l != 0)
        assert np.count_nonzero((rc > 0) & np.isinf(inst.l)) == 16 and np.count_nonzero((rc < 0) & np.isinf(inst.u)) == 55
        assert np.any((rc > 0) & box) and np.any((rc < 0) & box)


# ------------------------------------------------------------------------------------------ 2. the record
@pytest.mark.parametrize("warm", [True, False], ids=["warm", "cold"])
@pytest.mark.parametrize("name", ["A150", "A60", "B", "C"])
def test_the_record_describes_the_point_handed_back(ctx, name, warm):
    inst = case(name)
    forces_its_path(name, inst)
    lt = inst.sense == "<"
    x0, y0 = (inst.x, inst.y) if warm else (None, None)
    res, x, y = device(ctx, inst, x0, y0, LONGER[name], 1e-14)
    assert np.all(x >= inst.l) and np.all(x <= inst.u)           # (false for a NaN as well)
    assert np.all(y[lt] <= 0) and np.all(np.isfinite(y))
    same_record(f"{name} {'warm' if warm else 'cold'} longdouble", res, PC.record(inst.A, inst.b, inst.c, inst.l, inst.u, lt, x, y))
    m, n = inst.A.shape
    # sums of non-negative terms: (len + 2) eps bounds every order of summation, the square root included
    print(f"pdlp-edges {name} norms: b_norm={used(res.b_norm, np.linalg.norm(inst.b), (m + 2) * EPS):.3g} "
          f"c_norm={used(res.c_norm, np.linalg.norm(inst.c), (n + 2) * EPS):.3g}")
    assert float(res.b_norm) == pytest.approx(float(np.linalg.norm(inst.b)), rel=(m + 2) * EPS)
    assert float(res.c_norm) == pytest.approx(float(np.linalg.norm(inst.c)), rel=(n + 2) * EPS)
    if name == "B" and warm:
        assert x[5] == 0.0 and x[6] == 2.0                       # the empty columns sit at the bound their cost pushes them to


# ------------------------------------------------------------------------------------------ 3. the optimum
@pytest.mark.parametrize("name,fun", [("A150", -255.19659), ("B", -1390.54030)])
def test_optimum_against_highs(ctx, name, fun):
    inst = case(name)
    forces_its_path(name, inst)
    lt = inst.sense == "<"
    ref = PC.highs(inst)
    assert ref.fun == pytest.approx(fun, abs=1e-5)               # (the instance the recorded figures belong to)
    res, x, y = device(ctx, inst, inst.x, inst.y, 400000, 1e-9)
    print(f"pdlp-edges {name} converging run: status={int(res.status)} iters={int(res.iters)} restarts={int(res.restarts)} "
          f"primal_obj={used(res.primal_obj, ref.fun, 1e-6, 1e-6):.3g}")
    assert int(res.status) == 0
    assert float(res.primal_obj) == pytest.approx(ref.fun, rel=1e-6, abs=1e-6)
    r = inst.b - inst.A @ x
    assert np.abs(r[~lt]).max() < 1e-6 and r[lt].min() > -1e-6
    assert np.all(x >= inst.l) and np.all(x <= inst.u) and np.all(y[lt] <= 0)


# ------------------------------------------------------------------------------------------ 4. arguments
def same_bits(a, b):
    (ra, xa, ya), (rb, xb, yb) = a, b
    return (xa.tobytes() == xb.tobytes() and ya.tobytes() == yb.tobytes() and int(ra.iters) == int(rb.iters)
            and int(ra.status) == int(rb.status) and int(ra.restarts) == int(rb.restarts)
            and bytes(ra) == bytes(rb))


@pytest.mark.parametrize("name", ["c1", "A60"])
def test_no_row_mask_is_the_all_zero_mask(ctx, name):
    inst = case(name)
    m = inst.A.shape[0]
    none = device(ctx, inst, inst.x, inst.y, 128, 1e-14, lt=None)
    zero = device(ctx, inst, inst.x, inst.y, 128, 1e-14, lt=np.zeros(m, dtype=bool))
    assert same_bits(none, zero)
    assert np.all(np.isfinite(none[1])) and int(none[0].iters) == 128
    if np.any(inst.sense == "<"):                                 # ... and not the instance's own mask
        assert not same_bits(none, device(ctx, inst, inst.x, inst.y, 128, 1e-14))


@pytest.mark.parametrize("which", ["x0", "y0"])
@pytest.mark.parametrize("name", ["c1", "A60"])
def test_one_starting_vector_only(ctx, name, which):
    inst = case(name)
    x0, y0 = (inst.x, None) if which == "x0" else (None, inst.y)
    res, x, y = device(ctx, inst, x0, y0, 64, 1e-14)
    same_run(f"{name} {which} only", res, x, y, oracle(inst, x0, y0, 64), 64)


@pytest.mark.parametrize("name", ["c1", "A60"])
def test_iteration_limit_and_defaults(ctx, name):
    inst = case(name)
    res, x, y = device(ctx, inst, inst.x, inst.y, 100, 1e-14)
    assert int(res.iters) == 128 and int(res.status) == 3          # rounded up to whole periods of 64
    same_run(f"{name} max_iter=100", res, x, y, oracle(inst, inst.x, inst.y, 100), 128)
    dA = ctx.matrix(inst.A)
    try:
        # max_iter <= 0 is 20000, at a tolerance no run meets (so the limit is what ends it) and at one it meets before
        limit = device(ctx, inst, inst.x, inst.y, 0, 1e-30, A=dA)
        assert int(limit[0].iters) == 20032 and int(limit[0].status) == 3     # 20000 rounded up to a multiple of 64
        assert same_bits(limit, device(ctx, inst, inst.x, inst.y, 20000, 1e-30, A=dA))
        assert same_bits(limit, device(ctx, inst, inst.x, inst.y, -5, 1e-30, A=dA))
        default = device(ctx, inst, inst.x, inst.y, 0, 1e-8, A=dA)
        assert same_bits(default, device(ctx, inst, inst.x, inst.y, 20000, 1e-8, A=dA))
        assert int(default[0].status) == 0 and int(default[0].iters) < 20032
        assert same_bits(device(ctx, inst, inst.x, inst.y, 0, 0.0, A=dA), default)
        assert same_bits(device(ctx, inst, inst.x, inst.y, 0, -1.0, A=dA), default)
        assert not same_bits(device(ctx, inst, inst.x, inst.y, 0, 1e-6, A=dA), default)
    finally:
        dA.free()


def test_poll_interval_is_an_execution_detail(ctx, monkeypatch):
    inst = case("A60")
    monkeypatch.delenv("SX_PDLP_POLL", raising=False)
    default = device(ctx, inst, inst.x, inst.y, 400000, 1e-9)
    assert int(default[0].status) == 0 and int(default[0].iters) < 400000      # a converging run: the polls decide when it ends
    for poll in ("1", "3"):
        monkeypatch.setenv("SX_PDLP_POLL", poll)
        assert same_bits(device(ctx, inst, inst.x, inst.y, 400000, 1e-9), default), poll


def test_refusals_leave_the_context_usable(ctx):
    inst = case("A60")
    m, n = inst.A.shape
    shard = ctx.column_shard(sp.csc_matrix(inst.A))
    try:
        with pytest.raises(ValueError, match="both layouts"):
            device(ctx, inst, inst.x, inst.y, 64, 1e-14, A=shard)
    finally:
        shard.free()
    empty = workloads.LPInstance(A=sp.csr_matrix((0, n)), b=np.zeros(0), c=inst.c, l=inst.l, u=inst.u,
                                 sense=np.zeros(0, dtype="<U1"), x=inst.x, y=np.zeros(0))
    with pytest.raises(ValueError, match="empty problem"):
        device(ctx, empty, None, None, 64, 1e-14)
    res, x, y = device(ctx, inst, inst.x, inst.y, 64, 1e-14)
    same_run("A60 after the refusals", res, x, y, oracle(inst, inst.x, inst.y, 64), 64)
