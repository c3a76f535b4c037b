"""GPU: log-domain warm start on a separable pixel grid (sx_sinkhorn_grid_dev, one workgroup per image pair) against
POT's published `sinkhorn_log` restated in np.longdouble on the dense cost (tests/test_gpu_sinkhorn_log.py; POT is
absent -> parity unpinned), run on each instance's own support with M assembled from Cy and Cx.  Tolerances are the
project's: plans rtol 1e-9 (atol 1e-300), log-scalings rtol = atol = 1e-9, iteration counts within one test interval.
Measured on the CPU: a float64 numpy statement of the two-stage log-sum-exp differs from the longdouble reference on
the shapes below by at most 2.6e-12 in the log-scalings (|log-scaling| up to 1,000) and 3.5e-12 relative in the plan."""
import numpy as np
import pytest

import workloads
from test_gpu_sinkhorn import RTOL, grid_instances, marginals
from test_gpu_sinkhorn_log import check

pytestmark = pytest.mark.gpu


def instances(B, shape, seed, sparsity):
    """grid_instances for squares; the same masses on an H x W rectangle."""
    H, W = shape
    if H == W:
        return grid_instances(B, H, seed, sparsity)[:2]
    rng = np.random.default_rng(seed)
    a = rng.random((B, H * W)) * (rng.random((B, H * W)) > sparsity)
    b = rng.random((B, H * W)) * (rng.random((B, H * W)) > sparsity)
    a[:, 0] += 0.1
    b[:, -1] += 0.1
    return a / a.sum(axis=1, keepdims=True), b / b.sum(axis=1, keepdims=True)


def axis_costs(shape, power):
    return tuple(np.abs(np.subtract.outer(np.arange(k), np.arange(k))).astype(float) ** power for k in shape)


def check_on_own_support(plans, logs, a, b, M, reg, iters):
    for k in range(a.shape[0]):
        sa, sb = np.flatnonzero(a[k]), np.flatnonzero(b[k])
        sub = {"log_u": logs[k]["log_u"][sa], "log_v": logs[k]["log_v"][sb], "niter": logs[k]["niter"]}
        check(plans[k][np.ix_(sa, sb)], sub, a[k][sa], b[k][sb], M[np.ix_(sa, sb)], reg, iters)
        off = plans[k].copy()
        off[np.ix_(sa, sb)] = 0.0
        assert not off.any()                     # exactly zero (and no NaN) off the instance's support
        assert (logs[k]["log_u"][a[k] == 0] == -np.inf).all() and (logs[k]["log_v"][b[k] == 0] == -np.inf).all()


@pytest.mark.parametrize("shape,reg,iters,sparsity,power,B", [
    ((1, 1), 0.01, 50, 0.6, 1, 1), ((1, 7), 0.001, 50, 0.6, 1, 2), ((7, 1), 0.001, 50, 0.6, 1, 2),
    ((3, 5), 0.01, 200, 0.6, 1, 2),              # 200 iterations: two launches of 100
    ((9, 9), 0.005, 60, 0.6, 1, 2), ((28, 28), 0.005, 60, 0.8, 1, 2), ((17, 64), 0.05, 40, 0.6, 1, 1),
    ((33, 40), 1.0, 20, 0.6, 2, 1)])             # squared distances, handed over as a pair (Cy, Cx)
def test_plans_and_log_scalings_match_the_dense_algorithm(shape, reg, iters, sparsity, power, B):
    from smart_crossover.sinkhorn import sinkhorn_grid
    a, b = instances(B, shape, seed=B + shape[0] + shape[1], sparsity=sparsity)
    Cy, Cx = axis_costs(shape, power)
    n = shape[0] * shape[1]
    M = (Cy[:, None, :, None] + Cx[None, :, None, :]).reshape(n, n)
    plans, logs = sinkhorn_grid(a, b, shape, reg, numItermax=iters, log=True, cost="cityblock" if power == 1 else (Cy, Cx))
    assert plans.shape == (B, n, n)
    check_on_own_support(plans, logs, a, b, M, reg, iters)
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(logs[0]["u"], np.exp(logs[0]["log_u"]))
    # the one-instance form, and the named cost: the same bits (no atomics, fixed reduction order)
    one = sinkhorn_grid(a[0], b[0], shape, reg, numItermax=iters, cost="cityblock" if power == 1 else "sqeuclidean")
    np.testing.assert_array_equal(one, plans[0])


def test_more_than_sixteen_instances_in_one_call():
    from smart_crossover.sinkhorn import sinkhorn_grid
    a, b, M = grid_instances(19, 6, seed=25)
    plans, logs = sinkhorn_grid(a, b, (6, 6), 0.01, numItermax=60, log=True)
    check_on_own_support(plans, logs, a, b, M, 0.01, 60)


def test_agrees_with_the_dense_batched_log_method():
    from smart_crossover.sinkhorn import sinkhorn_batch, sinkhorn_grid
    a, b, _ = grid_instances(4, 10, seed=77)
    dense, dlogs = sinkhorn_batch(a, b, workloads.grid_cost(10), 0.02, numItermax=100, log=True, method="sinkhorn_log")
    got, glogs = sinkhorn_grid(a, b, (10, 10), 0.02, numItermax=100, log=True)
    np.testing.assert_allclose(got, dense, rtol=RTOL, atol=1e-300)
    assert all(abs(g["niter"] - d["niter"]) <= 10 for g, d in zip(glogs, dlogs)) and set(glogs[0]) == set(dlogs[0])


def test_grid_plan_feeds_the_crossover():
    """Disjoint thirds of the 12 x 12 grid at reg 0.005, as in test_gpu_sinkhorn_log.py: the grid plan, restricted to
    the two supports, starts TNET, which reaches linprog's optimal cost."""
    import io
    from contextlib import redirect_stdout
    from scipy.optimize import linprog
    from smart_crossover.formats import OptTransport
    from smart_crossover.network_methods.algorithms import network_crossover
    from smart_crossover.sinkhorn import sinkhorn_grid
    from smart_crossover.solver_caller.caller import SolverSettings
    col = np.arange(144) % 12
    src, snk = np.flatnonzero(col < 4), np.flatnonzero(col >= 8)
    a, b = np.zeros(144), np.zeros(144)
    a[src], b[snk] = marginals(src.size, snk.size, 12)
    M = workloads.grid_cost(12)[np.ix_(src, snk)]
    got = sinkhorn_grid(a, b, (12, 12), 0.005, numItermax=300)[np.ix_(src, snk)]
    ot = OptTransport(a[src].copy(), b[snk].copy(), M.copy())
    mcf = ot.to_MCF()
    ref = linprog(mcf.c, A_eq=mcf.A, b_eq=mcf.b, bounds=(0, None), method="highs")
    with redirect_stdout(io.StringIO()):
        out = network_crossover(got.flatten(), ot=ot, method="tnet", solver="HIP", solver_settings=SolverSettings(log_console=0))
    X = out.x.reshape(M.shape)
    assert float((X * M).sum()) == pytest.approx(ref.fun, rel=1e-8)
    assert np.allclose(X.sum(axis=1), a[src], atol=1e-8) and np.allclose(X.sum(axis=0), b[snk], atol=1e-8)


@pytest.mark.parametrize("shape,n,cost", [((1, 200), 200, "cityblock"),          # 200 * 201 + 1 + 800 > 20,000 doubles
                                          ((3, 5), 16, "cityblock"), ((3, 5), 15, "chebyshev")])
def test_bad_arguments_raise(shape, n, cost):
    from smart_crossover.sinkhorn import sinkhorn_grid
    with pytest.raises(ValueError):
        sinkhorn_grid(np.ones(n) / n, np.ones(n) / n, shape, 1.0, cost=cost)
