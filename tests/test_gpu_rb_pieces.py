"""GPU: the staged long rows of the column-blocked row layout (option "rb_stage_long", csrc/sx_rowblock.h) -- the
device builder's side arrays against their numpy statement (tools/rb_layout.py stage_long), and K2 / the CG row pass
through the pre-pass k_rb_long_products against the gathered layout, the plain walk and the CPU oracle, bit for bit."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT, bits_equal
from oracle import lp_path as L
import workloads

sys.path.insert(0, os.path.join(ROOT, "tools"))
import rb_layout as RB  # noqa: E402

pytestmark = pytest.mark.gpu

PARAMS = dict(R=512, cwin=4096, chunk=2048, dense_min=512, budget=96 * 512, merge_max=32768)


@pytest.fixture(scope="module")
def ctx():
    from smart_crossover.hip import Context
    c = Context(0)
    yield c
    c.set_option("rb_stage_long", -1)
    c.set_option("rowblock", -1)
    c.close()


def staircase(m, nb, window, seed=5):
    sh = workloads.lp_shard(0, 1, m=m, n_block=nb, k=8, seed=seed, structure="staircase", window=window)
    return sh.row_block, sh.x, sh.b, sh.y[:m]


def hand_made(seed=11):
    """Five long rows of 600 entries -- fewer long entries than one piece, all of one super-tile, a long-row count that
    is no multiple of 64 -- with duplicate columns inside them, among short rows; columns beyond 7000 are empty."""
    rng = np.random.default_rng(seed)
    m, n = 900, 9_000
    lens = rng.integers(0, 9, size=m)
    lens[100:105] = 600                                                 # consecutive: one super-tile
    cols = [np.sort(rng.integers(0, 7_000, size=k)) for k in lens]      # with replacement: duplicates
    A = sp.csr_matrix((rng.uniform(-1, 1, int(lens.sum())), np.concatenate(cols), np.concatenate([[0], np.cumsum(lens)])),
                      shape=(m, n))
    assert (np.diff(A.indptr) > 512).sum() == 5 and (np.diff(A[100].indices) == 0).any()
    return A, rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)


CASES = {"staircase_3000": lambda: staircase(3_000, 30_000, 64),
         "staircase_20000": lambda: staircase(20_000, 200_000, 512),
         "hand_made": hand_made}


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    A, x, b, y = CASES[request.param]()
    lay = RB.build(A, **PARAMS)
    return request.param, A, x, b, y, lay, RB.stage_long(lay)


def k2(ctx, dA, x, b, y, gamma_dual=1e-3):
    m = dA.shape[0]
    s_p, flag = ctx.empty(m, np.float64), ctx.empty(m, np.uint8)
    ctx.score_rows(dA, ctx.to_device(x), ctx.to_device(b), ctx.to_device(y), gamma_dual, s_p, flag)
    return s_p.download(), flag.download()


def matrix_with(ctx, A, rowblock, stage):
    ctx.set_option("rowblock", rowblock)
    ctx.set_option("rb_stage_long", stage)
    return ctx.matrix(A)


def test_device_side_arrays_equal_the_numpy_builder(ctx, case):
    name, A, x, b, y, lay, S = case
    dA = matrix_with(ctx, A, 1, 1)
    got = dA.rowblock(download=True)
    dA.free()
    assert got is not None and got["piece"] == S["piece"] == RB.PIECE
    assert (got["nl"], got["nls"]) == (S["nl"], S["nls"])
    if name == "staircase_3000":
        assert S["nl"] == 30_000 and lay["long_st"].sum() == 8          # three full pieces and a partial one; the
                                                                        # staircase's 8 regions bring 3 long rows each
    if name == "staircase_20000":
        assert S["nl"] == 200_000 and lay["long_st"].sum() == 8
    if name == "hand_made":
        assert S["nl"] == 3_000 < RB.PIECE and lay["long_st"].sum() == 1
    assert np.array_equal(got["chunks"]["staged"], S["staged"])
    for f in ("e0", "ne", "col0", "cell", "base", "fresh"):             # the main layout is the gathered one's
        assert np.array_equal(got["chunks"][f], lay["chunks"][f]), f
    assert np.array_equal(got["idx"], lay["idx"]) and bits_equal(got["val"], lay["val"])
    assert np.array_equal(got["lcol"], S["lcol"]) and bits_equal(got["lval"], S["lval"])
    assert np.array_equal(got["lperm"], S["lperm"])
    assert np.array_equal(got["lsrc"], S["lsrc"])


def special_x(A, x, seed):
    """x with -0.0, inf and nan at columns the long rows use."""
    rng = np.random.default_rng(seed)
    long_rows = np.flatnonzero(np.diff(A.indptr) > 512)
    cols = np.unique(np.concatenate([A.indices[A.indptr[r]:A.indptr[r + 1]] for r in long_rows]))
    pick = rng.choice(cols, size=9, replace=False)
    xs = x.copy()
    xs[pick[:3]], xs[pick[3:6]], xs[pick[6:]] = -0.0, np.inf, np.nan
    return xs


def test_k2_through_the_pieces_is_bit_identical(ctx, case):
    name, A, x, b, y, lay, S = case
    x2 = special_x(A, np.random.default_rng(17).standard_normal(A.shape[1]), 18)
    res = {}
    for key, (rbk, stage) in {"plain": (0, 0), "gather": (1, 0), "staged": (1, 1)}.items():
        dA = matrix_with(ctx, A, rbk, stage)
        first = k2(ctx, dA, x, b, y)
        second = k2(ctx, dA, x2, b, y)              # same matrix, another x: nothing is left over from the first call
        third = k2(ctx, dA, x, b, y)
        info = dA.rowblock()
        res[key] = (first, second, third, info)
        dA.free()
    assert res["plain"][3] is None and res["gather"][3]["nl"] == 0 and res["staged"][3]["nl"] == S["nl"] > 0
    for call, xx in ((0, x), (1, x2), (2, x)):
        want = L.primal_slack(A, b, xx)
        got = res["staged"][call]
        for other in ("plain", "gather"):
            assert bits_equal(got[0], res[other][call][0]) and np.array_equal(got[1], res[other][call][1]), (other, call)
        assert bits_equal(got[0], want), call
        assert np.array_equal(got[1], L.row_flags(want, y, 1e-3)), call
    assert np.isnan(res["staged"][1][0]).any()                           # the non-finite operands did reach long rows


def test_a_matrix_without_long_rows_takes_the_plain_path_of_the_layout(ctx):
    rng = np.random.default_rng(8)
    m, n, k = 2_000, 9_000, 12
    cols = np.sort(rng.integers(0, n, size=(m, k)), axis=1)
    A = sp.csr_matrix((rng.uniform(-1, 1, m * k), cols.ravel(), np.arange(m + 1) * k), shape=(m, n))
    x, b, y = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
    dA = matrix_with(ctx, A, 1, 1)
    got = k2(ctx, dA, x, b, y)
    info = dA.rowblock(download=True)
    dA.free()
    assert info is not None and info["nl"] == 0 and info["nls"] == 0 and "lsrc" not in info
    assert not info["chunks"]["staged"].any()
    assert bits_equal(got[0], b - L.seq_segment_sums(A.indptr, A.indices, A.data, x))


def test_auto_rule_keeps_the_gather_below_its_threshold(ctx):
    A, x, b, y = staircase(20_000, 200_000, 512)     # 2e5 long entries < 2^21
    dA = matrix_with(ctx, A, 1, -1)
    info = dA.rowblock()
    dA.free()
    assert info is not None and info["nl"] == 0


def test_projector_cg_row_pass_matches_through_the_pieces(ctx, case):
    """k_rb_cg_a over the staged layout (its pre-pass carries the CG's `done` early exit) on every input of the file:
    the 20,000-row staircase has a dozen chunks per long super-tile, the hand-made matrix less than one piece."""
    name, A, x, b, y, lay, S = case
    m, n = A.shape
    rng = np.random.default_rng(3)
    xa, xs, c = rng.uniform(0.1, 1, n), rng.uniform(0.1, 1, m), rng.standard_normal(n)
    out = {}
    for key, (rbk, stage) in {"plain": (0, 0), "gather": (1, 0), "staged": (1, 1)}.items():
        dA = matrix_with(ctx, A, rbk, stage)
        pc, pr = ctx.empty(n, np.float64), ctx.empty(m, np.float64)
        res = ctx.projector_norm(dA, ctx.to_device(xa), ctx.to_device(xs), ctx.to_device(c), 1e-10, 2000, pc, pr)
        info = dA.rowblock()
        out[key] = (res.proj_norm, int(res.iters), int(res.converged), pc.download(), pr.download(),
                    0 if info is None else 1 + info["nl"])
        dA.free()
    print(name, {k: v[:3] for k, v in out.items()})
    assert out["plain"][5] == 0 and out["gather"][5] == 1 and out["staged"][5] == 1 + S["nl"] > 1
    g, s, p = out["gather"], out["staged"], out["plain"]
    # same row sums, same block partials: the CG over the staged layout repeats the gathered one's history exactly
    assert s[1] == g[1] > 0 and s[2] == g[2] and s[0] == g[0]
    assert bits_equal(s[3], g[3]) and bits_equal(s[4], g[4])
    # ... and agrees with the plain walk as the layout itself does (other block partials: rounding only)
    assert s[2] == p[2] == 1 and s[0] == pytest.approx(p[0], rel=1e-9)
    np.testing.assert_allclose(s[3], p[3], rtol=1e-6, atol=1e-9 * np.abs(p[3]).max())
    np.testing.assert_allclose(s[4], p[4], rtol=1e-6, atol=1e-9 * max(np.abs(p[4]).max(), 1e-300))
