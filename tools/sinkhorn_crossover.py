#!/usr/bin/env python3
"""What a sharper entropic plan is worth to the OT crossover: on the side x side grid (28 = BASELINE config 3 size)
one instance pair, its warm start by each Sinkhorn method at several reg, and TNET from each plan -- iterations
(pushes + simplex) and wall time of network_crossover, objective against the first finished run.
    python tools/sinkhorn_crossover.py [--side 28] [--regs 10 1 0.1 0.02 0.005] [--iters 1000] [--methods sinkhorn sinkhorn_log]
--methods may name sinkhorn_grid (the separable-grid kernel, any iteration count at a usable cost).
"""
import argparse
import io
import json
import os
import sys
import time
import warnings
from contextlib import redirect_stdout

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "smart-crossover_amd"))

import workloads  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=28)
    ap.add_argument("--regs", type=float, nargs="+", default=[10.0, 1.0, 0.1, 0.02, 0.005])
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--methods", nargs="+", default=["sinkhorn", "sinkhorn_log"], choices=("sinkhorn", "sinkhorn_log", "sinkhorn_grid"))
    args = ap.parse_args()
    from smart_crossover.formats import OptTransport
    from smart_crossover.network_methods.algorithms import network_crossover
    from smart_crossover.sinkhorn import sinkhorn, sinkhorn_grid
    from smart_crossover.solver_caller.caller import SolverSettings
    n = args.side * args.side
    rng = np.random.default_rng(3)
    a, b = rng.random(n) + 0.05, rng.random(n) + 0.05
    a /= a.sum()
    b /= b.sum()
    M = workloads.grid_cost(args.side)

    def crossover(plan):
        ot = OptTransport(a.copy(), b.copy(), M.copy())
        t0 = time.perf_counter()
        with redirect_stdout(io.StringIO()):
            out = network_crossover(plan.flatten(), ot=ot, method="tnet", solver="HIP", solver_settings=SolverSettings(log_console=0))
        return {"crossover_s": time.perf_counter() - t0, "iterations": float(out.iter_count), "obj": float(out.obj_val)}

    rows = []
    warm = False
    for reg in args.regs:
        for method in args.methods:
            t0 = time.perf_counter()
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                if method == "sinkhorn_grid":
                    plan, log = sinkhorn_grid(a, b, (args.side, args.side), reg, numItermax=args.iters, log=True)
                else:
                    plan, log = sinkhorn(a, b, M, reg, numItermax=args.iters, log=True, method=method)
            row = {"reg": reg, "method": method, "sinkhorn_s": time.perf_counter() - t0, "niter": log["niter"],
                   "err": log["err"], "broke_down": any("numerical errors" in str(w.message) for w in caught), "plan_nonzeros": int(np.count_nonzero(plan))}
            try:
                if not warm:                     # the first crossover of a process loads code objects: not timed
                    crossover(plan)
                    warm = True
                row.update(crossover(plan))
            except ValueError as exc:            # TNET: the plan's support does not connect all nodes
                row["crossover_error"] = str(exc)
            rows.append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps({"side": args.side, "iters": args.iters, "rows": rows}))


if __name__ == "__main__":
    main()
