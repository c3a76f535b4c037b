#!/usr/bin/env python3
"""Entropic OT warm starts of B instance pairs on the 28 x 28 grid (BASELINE config 3 size, the reference's
driver loops over ten of them): one sx_sinkhorn_dev call per instance vs one sx_sinkhorn_batch_dev call.
    python tools/sinkhorn_bench.py [--B 10] [--reg 0.5] [--iters 1000] [--method sinkhorn|sinkhorn_log|both]
--method both alternates the two methods inside each repetition, so their figures come from one process.
    python tools/sinkhorn_bench.py --grid [--side 28] [--B 10] [--reg 0.5] [--iters 1000]
--grid times sx_sinkhorn_grid_dev (one workgroup per pair, no dense M) next to the batched log-domain call on the same
grid inputs, alternating; host clock around blocking calls, without a plan (per iteration) and with the plans
written and downloaded (whole call).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "smart-crossover_amd"))

import workloads  # noqa: E402


def grid_compare(args):
    from smart_crossover.hip.device import default_context
    ctx = default_context()
    side, B = args.side, args.B
    n = side * side
    rng = np.random.default_rng(3)
    a = rng.random((B, n)) + 0.05
    b = rng.random((B, n)) + 0.05
    a /= a.sum(axis=1, keepdims=True)
    b /= b.sum(axis=1, keepdims=True)
    C1 = np.abs(np.subtract.outer(np.arange(side), np.arange(side))).astype(np.float64)
    dM, dC = ctx.to_device(workloads.grid_cost(side).reshape(-1)), ctx.to_device(C1.reshape(-1))
    da, db = ctx.to_device(a.reshape(-1)), ctx.to_device(b.reshape(-1))
    d_u, d_v, d_plan = ctx.empty(B * n, np.float64), ctx.empty(B * n, np.float64), ctx.empty(B * n * n, np.float64)
    calls = {"sinkhorn_log": lambda plan: ctx.sinkhorn_log_batch(n, n, B, da, db, dM, args.reg, args.iters, 1e-9, plan, d_u, d_v),
             "sinkhorn_grid": lambda plan: ctx.sinkhorn_grid(side, side, B, da, db, dC, dC, args.reg, args.iters, 1e-9, plan, d_u, d_v)}
    rec = {"B": B, "grid": f"{side}x{side}", "reg": args.reg, "iters": args.iters, "clock": "host, blocking calls"}
    log_u = {}
    for rep in range(args.reps + 1):                # repetition 0 warms both methods up and is not recorded
        for name, call in calls.items():
            t0 = time.perf_counter()
            res = call(None)
            t1 = time.perf_counter()
            call(d_plan)
            plans = d_plan.download()
            t2 = time.perf_counter()
            log_u[name] = d_u.download()
            its = max(int(r.iters) for r in res)
            if rep:
                rec.setdefault(name, []).append({"iterations": its, "us_per_iteration": (t1 - t0) * 1e6 / max(its, 1),
                                                 "solve_ms": (t1 - t0) * 1e3, "whole_call_with_plans_ms": (t2 - t1) * 1e3,
                                                 "plan_row_sum_err": float(np.abs(plans.reshape(B, n, n).sum(axis=2) - a).max())})
    rec["max_abs_diff_log_u"] = float(np.abs(log_u["sinkhorn_grid"] - log_u["sinkhorn_log"]).max())
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", action="store_true", help="time sinkhorn_grid next to the batched log-domain method")
    ap.add_argument("--side", type=int, default=28, help="--grid: side of the pixel grid")
    ap.add_argument("--reps", type=int, default=3, help="--grid: recorded repetitions")
    ap.add_argument("--B", type=int, default=10)
    ap.add_argument("--reg", type=float, default=0.5, help="small: the loop runs to the iteration limit")
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--method", choices=("sinkhorn", "sinkhorn_log", "both"), default="sinkhorn")
    args = ap.parse_args()
    if args.grid:
        return grid_compare(args)
    methods = ("sinkhorn", "sinkhorn_log") if args.method == "both" else (args.method,)
    from smart_crossover.hip.device import default_context
    ctx = default_context()
    side = 28
    n = side * side
    rng = np.random.default_rng(3)
    a = rng.random((args.B, n)) + 0.05
    b = rng.random((args.B, n)) + 0.05
    a /= a.sum(axis=1, keepdims=True)
    b /= b.sum(axis=1, keepdims=True)
    M = workloads.grid_cost(side)
    dM = ctx.to_device(M.reshape(-1))
    da, db = ctx.to_device(a.reshape(-1)), ctx.to_device(b.reshape(-1))
    d_u, d_v = ctx.empty(args.B * n, np.float64), ctx.empty(args.B * n, np.float64)
    rec = {"B": args.B, "grid": f"{side}x{side}", "reg": args.reg, "iters": args.iters}
    for rep in range(2):
        for method in methods:
            single, batch = ((ctx.sinkhorn, ctx.sinkhorn_batch) if method == "sinkhorn" else
                             (ctx.sinkhorn_log, ctx.sinkhorn_log_batch))
            t0 = time.perf_counter()
            it_single = 0
            for k in range(args.B):
                ak = ctx.wrap(da.ptr + 8 * k * n, n, np.float64, owner=da)
                bk = ctx.wrap(db.ptr + 8 * k * n, n, np.float64, owner=db)
                r = single(n, n, ak, bk, dM, args.reg, args.iters, 1e-9, None,
                           ctx.wrap(d_u.ptr + 8 * k * n, n, np.float64, owner=d_u), ctx.wrap(d_v.ptr + 8 * k * n, n, np.float64, owner=d_v))
                it_single += int(r.iters)
            t1 = time.perf_counter()
            u_single = d_u.download()
            res = batch(n, n, args.B, da, db, dM, args.reg, args.iters, 1e-9, None, d_u, d_v)
            t2 = time.perf_counter()
            u_batch = d_u.download()
            it_batch = max(int(r.iters) for r in res)
            diff = np.abs(u_batch - u_single) / (np.abs(u_single) if method == "sinkhorn" else 1.0)   # log-scalings: absolute
            rec.setdefault(method, {})[f"run{rep}"] = {
                "single_calls_ms": (t1 - t0) * 1e3, "single_us_per_iteration_and_instance": (t1 - t0) * 1e6 / max(it_single, 1),
                "batch_ms": (t2 - t1) * 1e3, "batch_us_per_iteration": (t2 - t1) * 1e6 / max(it_batch, 1),
                "iterations_single_total": it_single, "iterations_batch": it_batch, "max_diff_u": float(np.max(diff))}
    for method in methods:
        r = rec[method]["run1"]
        if method == "sinkhorn":
            flop = 2 * 2.0 * n * n * 16               # two 784 x 784 x 16 products per iteration (16 = MFMA tile of instances)
            r["mfma_fp64_tflops"] = flop / (r["batch_us_per_iteration"] * 1e-6) / 1e12
        else:
            r["exp_per_second"] = 2.0 * n * n * args.B / (r["batch_us_per_iteration"] * 1e-6)   # one per element, pass and instance
        r["speedup_over_instance_loop"] = r["single_calls_ms"] / r["batch_ms"]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
