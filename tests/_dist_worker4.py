"""Worker of the gloo rehearsal of the column-sharded re-solve (TEST INFRASTRUCTURE): ShardedLP.restricted_resolve over
`world` ranks -- restricted LP replicated (solved by HiGHS here, by the device solvers on the GPU), pricing of the other
columns rank-local (played by the CPU oracle), one all-gather of the pricing records and one of the entering columns per
round; rank 0 writes the rounds' columns and the optimum."""
import dataclasses
import json
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "smart-crossover_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import workloads                               # noqa: E402
from smart_crossover import distributed as D   # noqa: E402
from smart_crossover.formats import GeneralLP  # noqa: E402
from _dist_ops import OracleOps                # noqa: E402


def problem(m=600, n=6000, seed=17):
    """A netlib-style LP and another cost vector, so that the columns the start leaves free are not the optimum's."""
    inst = workloads.netlib_lp(m, n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    c = inst.c + 0.3 * rng.standard_normal(n)
    u = np.where(np.isinf(inst.u), 30.0, inst.u)
    start = np.flatnonzero(inst.x > 1e-6)          # the interior columns of the point: a feasible restricted LP
    mode = os.environ.get("SX_TEST_BOUNDS")
    if mode in ("image", "image-open"):
        # the same LP under x = d * x' + t (tests/_general_bounds.py): non-zero resting bounds, boxes that straddle 0.
        # The start is chosen by the same rule: the columns the point does not leave at the bound they would rest at
        # outside the restricted LP (above, with l = 0: x > 1e-6) -- a mirrored column at its upper bound is among them
        from _general_bounds import affine_image, free_some, highs
        inst, _, _, _ = affine_image(dataclasses.replace(inst, c=c, u=u, x=np.clip(inst.x, inst.l, u)), 5)
        if mode == "image-open":
            # bounds that are not active at the optimum taken away (the optimum stays where it is): the columns at their
            # upper bound both at the point and at the optimum lose their lower bound -- UPPER-ONLY columns that rest at u
            # outside the restricted LP --, the columns at l = 0 at the point that the optimum holds strictly inside their
            # box lose both -- FREE columns that rest at 0 outside it and have to enter
            ref = highs(inst)
            assert ref.status == 0
            at_up = (np.abs(inst.u - inst.x) <= 1e-6) & (np.abs(inst.u - ref.x) <= 1e-9)
            inside = (inst.l == 0.0) & (np.abs(inst.x) <= 1e-6) & (ref.x > inst.l + 1e-3) & (ref.x < inst.u - 1e-3)
            l = inst.l.copy()
            l[at_up] = -np.inf
            inst = free_some(dataclasses.replace(inst, l=l), np.flatnonzero(inside))
        c, u = inst.c, inst.u
        start = np.flatnonzero(np.abs(inst.x - D.resting_bound(inst.l, inst.u)) > 1e-6)
    lp = GeneralLP(inst.A, inst.b, c, inst.l, u, inst.sense)
    problem.point = (inst.x, inst.y)
    return lp, start


def make_ops():
    if os.environ.get("SX_DIST_OPS", "oracle") == "hip":      # the real kernels, every rank on GPU 0 (tests/test_gpu_dist.py)
        import torch
        from smart_crossover.hip import Context
        torch.cuda.set_device(0)
        stream = torch.cuda.Stream()
        torch.cuda.set_stream(stream)
        return D.HipOps(Context(0, stream.cuda_stream), torch)
    return OracleOps()


def main():
    out_path, batch = sys.argv[1], int(os.environ.get("SX_TEST_BATCH", "64"))
    solver = os.environ.get("SX_TEST_SOLVER", "HGS")
    single = os.environ.get("WORLD_SIZE", "1") == "1"
    if not single:
        dist.init_process_group("gloo")
    size = [int(v) for v in os.environ.get("SX_TEST_SIZE", "600,6000").split(",")]
    lp, start = problem(*size)
    sh = D.ShardedLP(lp, None if single else dist, make_ops())
    trace = []
    kw = {}
    if solver == "HIP":      # the device's first solve starts at the point (first-order stage + sparse crossover), not at the slack basis
        kw = {"x_start": problem.point[0], "y_start": problem.point[1], "first_method": "barrier"}
    fail_rank = os.environ.get("SX_TEST_FAIL_RANK")
    if fail_rank is not None:    # one rank's replicated solve fails in its second round: every rank must leave, none may hang
        from smart_crossover.solver_caller import solving
        real, calls = solving.solve_lp, [0]

        def flaky(*a, **k):
            calls[0] += 1
            if calls[0] == 2 and (single or dist.get_rank() == int(fail_rank)):
                raise MemoryError("injected failure of the replicated solve")
            return real(*a, **k)
        solving.solve_lp = flaky
        rank = 0 if single else dist.get_rank()
        try:
            sh.restricted_resolve(start, solver=solver, batch=batch, opt_tol=1e-7, trace=trace, **kw)
            msg = "no exception"
        except Exception as exc:       # noqa: BLE001
            msg = f"{type(exc).__name__}: {exc}"
        with open(f"{out_path}.rank{rank}", "w") as f:
            json.dump({"raised": msg, "rounds_added": len(trace)}, f)
        if rank == 0:
            with open(out_path, "w") as f:
                json.dump({"done": True}, f)
        if not single:
            dist.barrier()
            dist.destroy_process_group()
        return
    x_R, y, R, basis, status, rounds = sh.restricted_resolve(start, solver=solver, batch=batch, opt_tol=1e-7, trace=trace, **kw)
    x_all = D.resting_bound(lp.l, lp.u)            # the columns outside R rest at a bound: c_N @ x_N is part of the objective
    x_all[R] = x_R
    res = {"world": 1 if single else dist.get_world_size(), "status": status, "rounds": rounds, "trace": trace,
           "obj": float(lp.c @ x_all), "R": [int(j) for j in R], "basic": [int(j) for j in R[basis.vbasis == 0]]}
    if single or dist.get_rank() == 0:
        with open(out_path, "w") as f:
            json.dump(res, f)
    if not single:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
