#!/usr/bin/env python3
"""Times the column-norm walk next to K1 on the config-5 ``lp_shard`` column block, in one process, with the
context's event timers: sx_column_norms_dev, the fused sx_score_norm_dev, the elementwise sx_score_norm_dev (norms
given) and sx_score_columns_dev, alternating, after a warm-up.  Prints a markdown note (ms, algorithmic GB/s, share
of the 8 TB/s HBM peak); ``--out`` also writes it to a file.

    python tools/norm_bench.py [--rounds 9] [--reps 20] [--out profiles/r05/norm_score.md] [--small]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "smart-crossover_amd"))

import workloads  # noqa: E402
from smart_crossover.hip import Context  # noqa: E402

PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--small", action="store_true", help="config-2 size (a rehearsal of the tool, not a measurement)")
    args = ap.parse_args()
    m, nb, k = (20_000, 100_000, 20) if args.small else (1_000_000, 10_000_000, 8)
    structure = "uniform" if args.small else "staircase"
    sh = workloads.lp_shard(0, 1, m=m, n_block=nb, k=k, structure=structure)
    ctx = Context(0)
    dC = ctx.column_shard(sh.col_block)
    nnz = sh.col_block.nnz
    d = {kk: ctx.to_device(getattr(sh, kk)) for kk in ("y", "x", "c", "l", "u")}
    sumsq, norm, score = (ctx.empty(nb, np.float64) for _ in range(3))
    s_d, code = ctx.empty(nb, np.float64), ctx.empty(nb, np.uint8)

    # algorithmic bytes: what the kernel has to move, from the shapes
    legs = {
        "sx_column_norms_dev (norm only)": (8 * nnz + 8 * (nb + 1) + 8 * nb,
                                            lambda: ctx.column_norms(dC, norm=norm)),
        "sx_score_norm_dev fused, gap": (8 * nnz + 8 * (nb + 1) + 8 * nb + 24 * nb,
                                         lambda: ctx.score_norm(dC, d["x"], d["l"], d["u"], "gap", score=score)),
        "sx_score_norm_dev from norms, gap": (5 * 8 * nb,
                                              lambda: ctx.score_norm(dC, d["x"], d["l"], d["u"], "gap", norm=norm, score=score)),
        "sx_score_columns_dev (K1: s_d + code)": (12 * nnz + 8 * (nb + 1) + 41 * nb + 8 * m,
                                                  lambda: ctx.score_columns(dC, d["y"], d["c"], d["x"], d["l"], d["u"], 1e-3, s_d, code)),
    }
    for _, run in legs.values():       # warm-up: code objects, K1's layouts and its one-off variant timing
        for _ in range(3):
            run()
    ctx.sync()
    times = {name: [] for name in legs}
    for _ in range(args.rounds):       # alternating, so that drift of the shared machine hits every leg alike
        for name, (_, run) in legs.items():
            ctx.timer_start()
            for _ in range(args.reps):
                run()
            times[name].append(ctx.timer_stop() / args.reps)
    fused = score.download()
    ctx.score_norm(dC, d["x"], d["l"], d["u"], "gap", norm=norm, score=score)
    same = bool(np.array_equal(fused.view(np.uint64), score.download().view(np.uint64)))

    dev = ctx.device_info()[0]
    lines = [f"# Column norms and the norm-scaled indicator next to K1 ({'config-2 size: REHEARSAL' if args.small else 'config 5'})", "",
             f"`tools/norm_bench.py` on {dev}: `lp_shard` column block ({structure}), m = {m:,}, n = {nb:,}, nnz = {nnz:,}; "
             f"{args.rounds} alternating rounds of {args.reps} calls per leg after a warm-up, context event timers "
             "(`sx_timer_start` / `sx_timer_stop`).  GB/s are algorithmic bytes (from the shapes) over the median time; "
             f"the share is of the {PEAK_GBS / 1000:.0f} TB/s HBM peak.", "",
             "| call | algorithmic MB | median ms | min ms | max ms | GB/s | share of peak |", "|---|---|---|---|---|---|---|"]
    for name, (nbytes, _) in legs.items():
        t = np.array(times[name])
        gbs = nbytes / np.median(t) / 1e6
        lines.append(f"| {name} | {nbytes / 1e6:.1f} | {np.median(t):.4f} | {t.min():.4f} | {t.max():.4f} | {gbs:.0f} | {gbs / PEAK_GBS:.1%} |")
    med = {name: float(np.median(t)) for name, t in times.items()}
    names = list(legs)
    lines += ["", f"Norm walk / K1 (median): {med[names[0]] / med[names[3]]:.2f}; fused indicator / K1: {med[names[1]] / med[names[3]]:.2f}.  "
              f"Fused and from-norms scores bit-identical: {same}."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    dC.free()
    ctx.close()


if __name__ == "__main__":
    main()
