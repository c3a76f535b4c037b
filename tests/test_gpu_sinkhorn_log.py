"""GPU: log-domain entropic OT warm start (sx_sinkhorn_log_dev / _batch_dev) against POT's published
`sinkhorn_log` restated below in np.longdouble (POT is absent -> parity unpinned).  The device reduces in another
order than numpy, so plans agree to the project's relative 1e-9 (atol 1e-300 covers subnormal entries) and the
log-scalings to rtol = atol = 1e-9.  Measured on the CPU: the same statement in float64 differs from the longdouble
one on the inputs of this file by at most 2.7e-11 absolute in the log-scalings (|log-scaling| up to 23,000) and by
4.7e-11 relative in the normal plan entries -- a margin of about 20 below the tolerance."""
import numpy as np
import pytest
from scipy.special import logsumexp

import workloads
from test_gpu_sinkhorn import RTOL, grid_instances, marginals

pytestmark = pytest.mark.gpu


def sinkhorn_log_ref(a, b, M, reg, numItermax, stopThr=1e-9, dtype=np.longdouble):
    """(plan, log-scaling u, log-scaling v, completed iterations) of POT's sinkhorn_log on positive marginals."""
    a, b, M = (np.asarray(x, dtype=dtype) for x in (a, b, M))
    Mr = M / (-dtype(reg))
    loga, logb = np.log(a), np.log(b)
    u, v = np.zeros(a.size, dtype), np.zeros(b.size, dtype)
    iters = 0
    for ii in range(numItermax):
        v = logb - logsumexp(Mr + u[:, None], axis=0)
        u = loga - logsumexp(Mr + v[None, :], axis=1)
        iters = ii + 1
        if ii % 10 == 0:
            err = np.linalg.norm(np.exp(Mr + u[:, None] + v[None, :]).sum(axis=0) - b)
            if not err >= stopThr:
                break
    return np.exp(Mr + u[:, None] + v[None, :]), u, v, iters


def thirds(side):
    """Sources = left third, sinks = right third of a side x side grid: supports that do not overlap."""
    col = np.arange(side * side) % side
    src, snk = np.flatnonzero(col < side // 3), np.flatnonzero(col >= side - side // 3)
    a, b = marginals(src.size, snk.size, side)
    return a, b, workloads.grid_cost(side)[np.ix_(src, snk)]


def integer_costs(S, D, seed):
    a, b = marginals(S, D, seed)
    return a, b, np.random.default_rng(seed + 10).integers(5, 25, size=(S, D)).astype(float)


def check(got, glog, a, b, M, reg, iters):
    want, u, v, n = sinkhorn_log_ref(a, b, M, reg, iters)
    np.testing.assert_allclose(got, want.astype(float), rtol=RTOL, atol=1e-300)
    np.testing.assert_allclose(glog["log_u"], u.astype(float), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(glog["log_v"], v.astype(float), rtol=1e-9, atol=1e-9)
    assert abs(glog["niter"] - n) <= 10         # the test fires at iterations 0, 10, ...: one interval at most


@pytest.mark.parametrize("make,reg,iters,plain_breaks", [
    (lambda: integer_costs(12, 15, 0), 0.01, 200, True), (lambda: integer_costs(65, 130, 1), 0.02, 200, False),
    (lambda: integer_costs(257, 64, 2), 0.02, 37, False), (lambda: integer_costs(1, 7, 3), 0.001, 50, True),
    (lambda: integer_costs(9, 1, 4), 0.001, 50, True), (lambda: thirds(12), 0.005, 300, True)])
def test_plan_and_log_scalings_match_the_restated_algorithm(make, reg, iters, plain_breaks):
    from smart_crossover.sinkhorn import sinkhorn
    a, b, M = make()
    if plain_breaks:                             # what is new: the default method gives up on these inputs
        with pytest.warns(UserWarning):
            sinkhorn(a, b, M, reg, numItermax=iters)
    got, glog = sinkhorn(a, b, M, reg, numItermax=iters, log=True, method="sinkhorn_log")
    check(got, glog, a, b, M, reg, iters)
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(glog["u"], np.exp(glog["log_u"]))


def test_agrees_with_the_plain_device_method_where_both_work():
    """After a full iteration the two methods hold the same plan in exact arithmetic: their starts (1/dim against
    0) only move a constant between u and v."""
    from smart_crossover.sinkhorn import sinkhorn
    a, b = marginals(100, 130, 3)
    M = np.random.default_rng(13).integers(0, 20, size=(100, 130)).astype(float)
    plain, plog = sinkhorn(a, b, M, 5.0, numItermax=1000, log=True)
    got, glog = sinkhorn(a, b, M, 5.0, numItermax=1000, log=True, method="sinkhorn_log")
    np.testing.assert_allclose(got, plain, rtol=RTOL, atol=1e-300)
    assert abs(glog["niter"] - plog["niter"]) <= 10


def test_zero_masses_drop_out_without_nan():
    from smart_crossover.sinkhorn import sinkhorn
    a = np.array([0.6, 0.0, 0.4])
    b = np.array([0.0, 0.7, 0.0, 0.3])
    M = np.array([[0.0, 3300.0, 7.0, 1200.0], [5.0, 1.0, 2.0, 3.0], [2500.0, 40.0, 3300.0, 0.5]])
    got, glog = sinkhorn(a, b, M, 1.0, numItermax=100, log=True, method="sinkhorn_log")
    sa, sb = np.flatnonzero(a), np.flatnonzero(b)
    assert not np.isnan(got).any() and not np.isnan(glog["log_u"]).any() and not np.isnan(glog["log_v"]).any()
    assert not got[1].any() and not got[:, [0, 2]].any()
    assert glog["log_u"][1] == -np.inf and (glog["log_v"][[0, 2]] == -np.inf).all()
    sub = {"log_u": glog["log_u"][sa], "log_v": glog["log_v"][sb], "niter": glog["niter"]}
    check(got[np.ix_(sa, sb)], sub, a[sa], b[sb], M[np.ix_(sa, sb)], 1.0, 100)


@pytest.mark.parametrize("B,side,reg", [(3, 9, 0.005), (16, 12, 0.02), (1, 7, 0.001), (19, 6, 0.01)])
def test_batched_instances_match_the_algorithm_on_their_own_support(B, side, reg):
    from smart_crossover.sinkhorn import sinkhorn_batch
    a, b, M = grid_instances(B, side, seed=B + side)
    plans, logs = sinkhorn_batch(a, b, M, reg, numItermax=60, log=True, method="sinkhorn_log")
    for k in range(B):
        sa, sb = np.flatnonzero(a[k]), np.flatnonzero(b[k])
        sub = {"log_u": logs[k]["log_u"][sa], "log_v": logs[k]["log_v"][sb], "niter": logs[k]["niter"]}
        check(plans[k][np.ix_(sa, sb)], sub, a[k][sa], b[k][sb], M[np.ix_(sa, sb)], reg, 60)
        off = plans[k].copy()
        off[np.ix_(sa, sb)] = 0.0
        assert not off.any()                     # exactly zero (and no NaN) off the instance's support


def test_log_plan_feeds_the_crossover_where_the_plain_method_gives_nothing():
    """Disjoint thirds of the 12 x 12 grid at reg 0.005: TNET (method="tnet": the plan's support, 1,200 of 2,304
    entries, connects all nodes) started from the log plan reaches linprog's optimal cost; bounds as in
    test_gpu_sinkhorn.py::test_config3_warm_start_feeds_the_crossover."""
    import io
    from contextlib import redirect_stdout
    from scipy.optimize import linprog
    from smart_crossover.formats import OptTransport
    from smart_crossover.network_methods.algorithms import network_crossover
    from smart_crossover.sinkhorn import sinkhorn
    from smart_crossover.solver_caller.caller import SolverSettings
    a, b, M = thirds(12)
    got = sinkhorn(a, b, M, 0.005, numItermax=300, method="sinkhorn_log")
    ot = OptTransport(a.copy(), b.copy(), M.copy())
    mcf = ot.to_MCF()
    ref = linprog(mcf.c, A_eq=mcf.A, b_eq=mcf.b, bounds=(0, None), method="highs")
    with redirect_stdout(io.StringIO()):
        out = network_crossover(got.flatten(), ot=ot, method="tnet", solver="HIP", solver_settings=SolverSettings(log_console=0))
    X = out.x.reshape(M.shape)
    assert float((X * M).sum()) == pytest.approx(ref.fun, rel=1e-8)
    assert np.allclose(X.sum(axis=1), a, atol=1e-8) and np.allclose(X.sum(axis=0), b, atol=1e-8)


def test_unknown_method_raises():
    from smart_crossover.sinkhorn import sinkhorn, sinkhorn_batch
    with pytest.raises(ValueError):
        sinkhorn(np.ones(3) / 3, np.ones(4) / 4, np.zeros((3, 4)), 1.0, method="nope")
    with pytest.raises(ValueError):
        sinkhorn_batch(np.ones((2, 3)) / 3, np.ones((2, 4)) / 4, np.zeros((3, 4)), 1.0, method="nope")
