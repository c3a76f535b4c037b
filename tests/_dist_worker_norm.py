"""Worker of the norm-indicator tests: one rank of ``ShardedLP.norm_indicator`` / ``top_columns``
(smart_crossover/distributed.py).
  SX_DIST_OPS=oracle (default): a gloo rank, the rank-local kernel played by tests/_norm_oracle.py
                                (tests/test_norm_score_cpu.py);
  SX_DIST_OPS=hip:              no process group -- ``ShardedLP(lp, dist=None)`` on the GPU, created before any
                                other device call so that torch initialises HIP first, compared with a
                                single-context call (tests/test_gpu_norm_score.py)."""
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "smart-crossover_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch                                    # noqa: E402

import _norm_oracle as NO                       # noqa: E402
from _dist_ops import OracleOps                 # noqa: E402
from smart_crossover import distributed as D    # noqa: E402
from smart_crossover.formats import GeneralLP   # noqa: E402

K_TOP = (1, 40, 150)


class NormOracleOps(OracleOps):
    def norm_score(self, A, x, l, u, numerator):
        return torch.from_numpy(NO.norm_score(A.csr, x.numpy(), l.numpy(), u.numpy(), numerator)["score"].copy())


def problem():
    """60 x 421 LP whose columns 0, 3, 6, ... are one and the same column with the same x, l, u: their indicators tie,
    and the run of ties crosses every rank boundary of a 2- and a 3-rank split.  Some columns are free, some empty,
    some x lie outside their bounds."""
    rng = np.random.default_rng(11)
    m, n = 60, 421
    A = sp.random(m, n, density=0.08, random_state=np.random.RandomState(5), format="lil")
    same = sp.random(m, 1, density=0.2, random_state=np.random.RandomState(6), format="lil")
    same = same * 0.01                           # a small norm: the tied columns rank near the top
    for j in range(0, n, 3):
        A[:, j] = same
    for j in (1, 200, n - 1):
        A[:, j] = 0.0
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    l = np.where(rng.random(n) < 0.2, -np.inf, rng.uniform(-1.0, 0.0, n))
    u = np.where(rng.random(n) < 0.2, np.inf, rng.uniform(1.0, 2.0, n))
    x = rng.uniform(-1.2, 2.2, n)
    x[::3], l[::3], u[::3] = 0.25, 0.0, 1.0
    lp = GeneralLP(A, np.ones(m), np.ones(n), l, u, np.full(m, "="))
    return lp, x


def main():
    out_path = sys.argv[1]
    lp, x = problem()
    hip = os.environ.get("SX_DIST_OPS", "oracle") == "hip"
    if hip:
        dist, rank, world = None, 0, 1
        slp = D.ShardedLP(lp)                   # HipOps on torch's stream: before any other device call
        ops = slp.ops
    else:
        import torch.distributed as dist
        dist.init_process_group("gloo")
        rank, world = dist.get_rank(), dist.get_world_size()
        ops = NormOracleOps()
        slp = D.ShardedLP(lp, dist, ops)
    res = {"world": world, "blocks": [[b.start, b.stop] for b in slp.col_blocks]}
    for which in ("gap", "abs"):
        ind_loc = ops.host(slp.norm_indicator(x, which)).copy()
        tops = [slp.top_columns(k) for k in K_TOP]
        if dist is not None:
            gathered = [None] * world
            dist.all_gather_object(gathered, (slp.cols.start, ind_loc))
        else:
            gathered = [(slp.cols.start, ind_loc)]
        if rank == 0:
            ind = np.concatenate([g[1] for g in sorted(gathered, key=lambda g: g[0])])
            want = NO.norm_score(lp.A, x, lp.l, lp.u, which)["score"]
            order = NO.rank_desc(want)
            r = {"ind_bits_equal": bool(np.array_equal(ind.view(np.uint64), want.view(np.uint64))),
                 "top_equal": [bool(np.array_equal(t, order[:k])) for t, k in zip(tops, K_TOP)],
                 "ties_in_top": int(np.count_nonzero(want[order[:K_TOP[-1]]] == want[0]))}
            if hip:
                from smart_crossover.hip import Context
                ctx = Context(0)
                dA = ctx.matrix(lp.A)
                one = ctx.score_norm(dA, ctx.to_device(x), ctx.to_device(lp.l), ctx.to_device(lp.u), which).download()
                r["single_context_bits_equal"] = bool(np.array_equal(ind.view(np.uint64), one.view(np.uint64)))
                dA.free()
                ctx.close()
            res[which] = r
    if rank == 0:
        with open(out_path, "w") as f:
            json.dump(res, f)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
