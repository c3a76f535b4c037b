"""Entropic optimal-transport warm start on the device.

The reference's driver produces the inexact plan that TNET / CNET_OT start from with POT:
``sinkhorn(ot.s, ot.d, ot.M, reg=10, numItermax=1000)`` (scripts/run_network_crossover.py:95-97).  This
module offers the same call -- same argument names and defaults as ``ot.sinkhorn`` for the arguments the
reference uses -- computed by ``sx_sinkhorn_dev`` (csrc/sx_sinkhorn.hip).  POT is a third-party package
that is neither vendored nor pinned by the reference, so parity is unpinned; the tests compare with a
restatement of POT's published ``sinkhorn_knopp`` (oracle/sinkhorn.py).

``method="sinkhorn_log"`` runs POT's log-domain iteration instead (``sx_sinkhorn_log_dev``,
csrc/sx_sinkhorn_log.hip): the same plan in exact arithmetic, and still a plan when ``reg`` is so small that
``exp(-M/reg)`` underflows and the default method stops at iteration 0 with a warning.

``sinkhorn_grid`` runs the same log-domain iteration for image pairs on a pixel grid with a separable cost
(``sx_sinkhorn_grid_dev``, csrc/sx_sinkhorn_grid.hip): no dense ``M``, any number of pairs per call.
"""
from __future__ import annotations

import warnings
from typing import Tuple, Union

import numpy as np


METHODS = ("sinkhorn", "sinkhorn_log")


def _log_dict(log_u: np.ndarray, log_v: np.ndarray, res) -> dict:
    with np.errstate(over="ignore"):             # a log-scaling above 709 has no double: inf, as POT reports it
        return {"log_u": log_u, "log_v": log_v, "u": np.exp(log_u), "v": np.exp(log_v), "niter": int(res.iters),
                "err": float(res.err)}


def sinkhorn(a: np.ndarray, b: np.ndarray, M: np.ndarray, reg: float, numItermax: int = 1000, stopThr: float = 1e-9,
             log: bool = False, method: str = "sinkhorn") -> Union[np.ndarray, Tuple[np.ndarray, dict]]:
    """Sinkhorn-Knopp plan ``diag(u) exp(-M/reg) diag(v)`` for marginals ``a`` (sources) and ``b``
    (targets); with ``log=True`` also a dict with ``u``, ``v``, ``niter`` and the last tested ``err``.
    ``method="sinkhorn_log"`` iterates on the log-scalings (any ``reg > 0``); its dict also has ``log_u``, ``log_v``."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    from smart_crossover.hip.device import default_context
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    M = np.ascontiguousarray(M, dtype=np.float64)
    if M.shape != (a.size, b.size):
        raise ValueError("M must have shape (len(a), len(b))")
    ctx = default_context()
    S, D = M.shape
    plan, u, v = ctx.empty(S * D, np.float64), ctx.empty(S, np.float64), ctx.empty(D, np.float64)
    if method == "sinkhorn_log":
        res = ctx.sinkhorn_log(S, D, ctx.to_device(a), ctx.to_device(b), ctx.to_device(M.reshape(-1)), reg, numItermax,
                               stopThr, plan, u, v)
        if res.status == 2:
            warnings.warn(f"Warning: numerical errors at iteration {int(res.iters)}")
        out = plan.download().reshape(S, D)
        return (out, _log_dict(u.download(), v.download(), res)) if log else out
    res = ctx.sinkhorn(S, D, ctx.to_device(a), ctx.to_device(b), ctx.to_device(M.reshape(-1)), reg, numItermax, stopThr,
                       plan, u, v)
    if res.status == 2:
        warnings.warn(f"Warning: numerical errors at iteration {int(res.iters)}")
    out = plan.download().reshape(S, D)
    if log:
        return out, {"u": u.download(), "v": v.download(), "niter": int(res.iters), "err": float(res.err)}
    return out


def sinkhorn_batch(a: np.ndarray, b: np.ndarray, M: np.ndarray, reg: float, numItermax: int = 1000,
                   stopThr: float = 1e-9, log: bool = False, method: str = "sinkhorn"):
    """The warm starts of several instance pairs that share one cost matrix -- the reference's driver loops over
    ten MNIST image pairs on the same pixel grid (scripts/run_network_crossover.py:95-101) -- in one go:
    ``a`` is (B, S), ``b`` is (B, D), ``M`` is (S, D); a grid point an instance does not use carries mass 0 and
    drops out of that instance exactly as if it had been removed from its support.  Returns the (B, S, D) plans;
    with ``log=True`` also a list of dicts (``u``, ``v``, ``niter``, ``err``) per instance.  Batches of up to 16
    instances run as dense products on the fp64 matrix cores (``sx_sinkhorn_batch_dev``);
    ``method="sinkhorn_log"`` runs them through the log-domain kernels (``sx_sinkhorn_log_batch_dev``), where an
    unused grid point has log-scaling ``-inf``."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    from smart_crossover.hip.device import default_context
    a = np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64)
    b = np.ascontiguousarray(np.atleast_2d(b), dtype=np.float64)
    M = np.ascontiguousarray(M, dtype=np.float64)
    B = a.shape[0]
    if b.shape[0] != B or M.shape != (a.shape[1], b.shape[1]):
        raise ValueError("a must be (B, S), b (B, D) and M (S, D)")
    ctx = default_context()
    S, D = M.shape
    dM = ctx.to_device(M.reshape(-1))
    plans = np.empty((B, S, D))
    logs = []
    for lo in range(0, B, 16):
        nb = min(16, B - lo)
        d_plan, d_u, d_v = ctx.empty(nb * S * D, np.float64), ctx.empty(nb * S, np.float64), ctx.empty(nb * D, np.float64)
        run = ctx.sinkhorn_log_batch if method == "sinkhorn_log" else ctx.sinkhorn_batch
        res = run(S, D, nb, ctx.to_device(a[lo:lo + nb].reshape(-1)), ctx.to_device(b[lo:lo + nb].reshape(-1)),
                  dM, reg, numItermax, stopThr, d_plan, d_u, d_v)
        plans[lo:lo + nb] = d_plan.download().reshape(nb, S, D)
        u, v = d_u.download().reshape(nb, S), d_v.download().reshape(nb, D)
        for k, r in enumerate(res):
            if r.status == 2:
                warnings.warn(f"Warning: numerical errors at iteration {int(r.iters)} (instance {lo + k})")
            logs.append(_log_dict(u[k], v[k], r) if method == "sinkhorn_log" else
                        {"u": u[k], "v": v[k], "niter": int(r.iters), "err": float(r.err)})
    return (plans, logs) if log else plans


GRID_PLAN_BYTES = 1 << 30        # device plan buffer of one sinkhorn_grid call: larger batches are cut into several


def _axis_costs(shape, cost):
    H, W = shape
    if isinstance(cost, str):
        if cost not in ("cityblock", "sqeuclidean"):
            raise ValueError(f"cost must be 'cityblock', 'sqeuclidean' or a pair (Cy, Cx), not {cost!r}")
        power = 1 if cost == "cityblock" else 2
        return tuple(np.abs(np.subtract.outer(np.arange(k), np.arange(k))).astype(np.float64) ** power for k in (H, W))
    try:
        Cy, Cx = (np.ascontiguousarray(c, dtype=np.float64) for c in cost)
    except (TypeError, ValueError):
        raise ValueError("cost must be 'cityblock', 'sqeuclidean' or a pair (Cy, Cx)") from None
    if Cy.shape != (H, H) or Cx.shape != (W, W):
        raise ValueError("Cy must be (H, H) and Cx (W, W)")
    return Cy, Cx


def sinkhorn_grid(a: np.ndarray, b: np.ndarray, shape: Tuple[int, int], reg: float, numItermax: int = 1000,
                  stopThr: float = 1e-9, log: bool = False, cost="cityblock"):
    """Log-domain warm starts of image pairs on an ``H x W`` pixel grid whose cost is separable,
    ``M[(y,x),(y',x')] = Cy[y,y'] + Cx[x,x']`` -- the ``|dy| + |dx|`` of scripts/mnist2ot.py:30-40 (``"cityblock"``),
    squared distances (``"sqeuclidean"``) or any pair ``(Cy, Cx)`` -- without ever building ``M``: one workgroup
    iterates one pair in LDS (``sx_sinkhorn_grid_dev``, csrc/sx_sinkhorn_grid.hip), any number of pairs per call.
    ``a`` and ``b`` are ``(H*W,)`` or ``(B, H*W)``, row-major over the grid, mass 0 = pixel not used.  Returns what
    ``sinkhorn(..., method="sinkhorn_log")`` / ``sinkhorn_batch(..., method="sinkhorn_log")`` return for the dense
    ``M``.  Batches are cut so that the device plan buffer stays within ``GRID_PLAN_BYTES`` (1 GiB).  A grid beyond
    the kernel's limit (``W*(W|1) + H*(H|1) + 4*H*W <= 20000``; 56 x 56 fits) raises ``ValueError``."""
    from smart_crossover.hip.device import default_context
    try:
        H, W = (int(k) for k in shape)
    except (TypeError, ValueError):
        raise ValueError("shape must be (H, W)") from None
    single = np.ndim(a) == 1
    a = np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64)
    b = np.ascontiguousarray(np.atleast_2d(b), dtype=np.float64)
    n = H * W
    if H < 1 or W < 1 or a.ndim != 2 or a.shape[1] != n or b.shape != a.shape:
        raise ValueError("a and b must be (H*W,) or (B, H*W) for shape = (H, W)")
    Cy, Cx = _axis_costs((H, W), cost)
    ctx = default_context()
    dCy, dCx = ctx.to_device(Cy.reshape(-1)), ctx.to_device(Cx.reshape(-1))
    B = a.shape[0]
    chunk = max(1, min(B, GRID_PLAN_BYTES // (8 * n * n)))
    plans = np.empty((B, n, n))
    logs = []
    for lo in range(0, B, chunk):
        nb = min(chunk, B - lo)
        d_plan, d_u, d_v = ctx.empty(nb * n * n, np.float64), ctx.empty(nb * n, np.float64), ctx.empty(nb * n, np.float64)
        try:
            res = ctx.sinkhorn_grid(H, W, nb, ctx.to_device(a[lo:lo + nb].reshape(-1)), ctx.to_device(b[lo:lo + nb].reshape(-1)),
                                    dCy, dCx, reg, numItermax, stopThr, d_plan, d_u, d_v)
        except NotImplementedError as exc:       # SX_ERR_UNSUPPORTED: the grid does not fit the LDS of one CU
            raise ValueError(str(exc)) from None
        plans[lo:lo + nb] = d_plan.download().reshape(nb, n, n)
        u, v = d_u.download().reshape(nb, n), d_v.download().reshape(nb, n)
        for k, r in enumerate(res):
            if r.status == 2:
                warnings.warn(f"Warning: numerical errors at iteration {int(r.iters)}" + ("" if single else f" (instance {lo + k})"))
            logs.append(_log_dict(u[k], v[k], r))
    if single:
        return (plans[0], logs[0]) if log else plans[0]
    return (plans, logs) if log else plans
