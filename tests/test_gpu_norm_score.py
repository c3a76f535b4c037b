"""GPU: column norms and the optional norm-scaled column indicator (sx_column_norms_dev, sx_score_norm_dev,
sx_score_norm; include/sxhip.h K17) against the NumPy statement of their arithmetic (tests/_norm_oracle.py).
Everything is compared bit for bit: sumsq, norm (so the device sqrt against np.sqrt) and the score for both numerators."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import bits_equal, csr_from

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _norm_oracle as NO  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from smart_crossover.hip import Context
    c = Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ inputs
def vectors(n, seed):
    """x, l, u with every numerator case: lower / upper / both bounds infinite (free columns take |x|), x outside
    its bounds (negative score), x = NaN in one column."""
    rng = np.random.default_rng(seed)
    l = rng.uniform(-2.0, 0.0, n)
    u = l + rng.uniform(0.5, 3.0, n)
    x = rng.uniform(l, u)
    kind = rng.integers(0, 8, n)
    l[kind == 0] = -np.inf
    u[kind == 1] = np.inf
    l[kind == 2], u[kind == 2] = -np.inf, np.inf
    x[kind == 2] = rng.standard_normal(np.count_nonzero(kind == 2)) * 3.0
    out = kind == 3
    x[out] = np.where(rng.random(np.count_nonzero(out)) < 0.5, l[out] - 0.75, u[out] + 1.25)
    if n > 2:
        x[n // 2] = np.nan
    return x, l, u


def raw_csr(m, n, rows, cols, vals):
    """CSR with the entries of every row in the given order: inner indices unsorted, duplicates kept."""
    order = np.argsort(rows, kind="stable")
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))])
    return sp.csr_matrix((vals[order], cols[order], indptr), shape=(m, n))


def with_column_lengths(m, lengths, seed, value=None):
    """m x len(lengths) matrix whose column j has lengths[j] entries (distinct rows)."""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([rng.choice(m, k, replace=False) for k in lengths] + [np.zeros(0, dtype=np.int64)])
    cols = np.repeat(np.arange(len(lengths)), lengths)
    vals = rng.standard_normal(rows.size) if value is None else value(rng, rows.size)
    return sp.csr_matrix(sp.coo_matrix((vals, (rows, cols)), shape=(m, len(lengths))))


def long_column():
    """9,100 x 600: three entries, then ONE column of 9,001 entries -- longer than the 4,096-entry chunk and the
    8,192-entry tile budget, starting at an odd offset and straddling two chunk boundaries -- then short columns."""
    rng = np.random.default_rng(41)
    lengths = np.concatenate([[3, 9001], rng.integers(0, 8, 598)])
    return with_column_lengths(9100, lengths, 42)


def empties():
    """Empty columns first, last and in runs across the 256-column tile boundaries."""
    rng = np.random.default_rng(43)
    lengths = rng.integers(1, 9, 600)
    for a, b in ((0, 3), (250, 263), (505, 530), (597, 600)):
        lengths[a:b] = 0
    return with_column_lengths(80, lengths, 44)


def duplicates_unsorted():
    rng = np.random.default_rng(45)
    m, n, nnz = 120, 301, 5000
    rows, cols = rng.integers(0, m, nnz), rng.integers(0, n, nnz)
    cols[:1500] = rng.integers(0, 5, 1500)
    A = raw_csr(m, n, rows, cols, rng.choice([-1.0, 1.0], nnz) * 10.0 ** rng.uniform(-8, 8, nnz))
    assert not A.has_sorted_indices and A.nnz == nnz
    return A


def extreme_values():
    """Values from 1e-170 to 1e160: squares underflow to subnormals or zero and overflow to inf, so q == 0 (with
    entries present) and q == inf both occur."""
    def value(rng, k):
        return rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(-170, 160, k)
    rng = np.random.default_rng(46)
    lengths = rng.integers(0, 6, 700)
    A = with_column_lengths(64, lengths, 47, value).tolil()
    A[:, 5] = 0.0
    A[3, 5], A[9, 5] = 1e-170, -3e-165                      # q == 0 although the column has entries
    A[:, 6] = 0.0
    A[1, 6] = 1.5e-155                                       # q subnormal
    A[:, 7] = 0.0
    A[2, 7], A[4, 7] = 1e160, 1.0                            # q == inf
    return sp.csr_matrix(A)


def sqrt_inputs():
    """10,000 columns of one to three entries with a random exponent per column: q with random mantissas over
    2^-600 .. 2^600, odd and even exponents alike."""
    rng = np.random.default_rng(48)
    n = 10_000
    lengths = rng.integers(1, 4, n)
    scale = np.repeat(2.0 ** rng.integers(-300, 300, n), lengths)
    rows = np.concatenate([rng.choice(16, k, replace=False) for k in lengths])
    vals = rng.uniform(1.0, 2.0, rows.size) * scale
    return sp.csr_matrix(sp.coo_matrix((vals, (rows, np.repeat(np.arange(n), lengths))), shape=(16, n)))


def random_n(n):
    return sp.random(40, n, density=0.2, random_state=np.random.RandomState(100 + n), format="csr")


CASES = {
    "long_column": long_column,
    "n1": lambda: random_n(1),
    "n257": lambda: random_n(257),
    "n513": lambda: random_n(513),
    "empties": empties,
    "nnz0": lambda: sp.csr_matrix((7, 300)),
    "n0": lambda: sp.csr_matrix((5, 0)),
    "duplicates_unsorted": duplicates_unsorted,
    "extreme_values": extreme_values,
    "sqrt_inputs": sqrt_inputs,
}


# ------------------------------------------------------------------------------------------------ the comparison
def device_results(ctx, dA, x, l, u):
    """Everything the entry points compute for one matrix: norms, and per numerator the fused score, the score from
    given norms and the host-pointer variant."""
    from smart_crossover.hip import lib as sxl
    n = dA.shape[1]
    dx, dl, du = ctx.to_device(x), ctx.to_device(l), ctx.to_device(u)
    sumsq, norm = ctx.empty(n, np.float64), ctx.empty(n, np.float64)
    ctx.column_norms(dA, sumsq, norm)
    only_norm = ctx.empty(n, np.float64)
    ctx.column_norms(dA, norm=only_norm)
    out = dict(sumsq=sumsq.download(), norm=norm.download(), only_norm=only_norm.download())
    for which in ("gap", "abs"):
        bounds = (dl, du) if which == "gap" else (None, None)      # l and u may be NULL for SX_NORM_ABS
        out[which + "_fused"] = ctx.score_norm(dA, dx, bounds[0], bounds[1], which).download()
        out[which + "_from_norm"] = ctx.score_norm(dA, dx, bounds[0], bounds[1], which, norm=norm).download()
        host = np.full(n, 7.0)
        code = {"abs": sxl.NORM_ABS, "gap": sxl.NORM_GAP}[which]
        p = lambda a: a.ctypes.data                                  # noqa: E731
        sxl.check(ctx._lib.sx_score_norm(ctx.handle, dA.handle, p(x), p(l) if which == "gap" else None,
                                         p(u) if which == "gap" else None, code, None, p(host)))
        out[which + "_host"] = host
    return out


def assert_matches_oracle(got, A, x, l, u, sumsq_want=None):
    want = NO.norm_score(A, x, l, u, "gap")
    if sumsq_want is not None:
        assert np.array_equal(want["sumsq"].view(np.uint64), sumsq_want.view(np.uint64))
    assert bits_equal(got["sumsq"], want["sumsq"])
    assert bits_equal(got["norm"], want["norm"]) and bits_equal(got["only_norm"], want["norm"])
    for which in ("gap", "abs"):
        score = NO.score_from_sumsq(want["sumsq"], x, l, u, which)
        for path in ("_fused", "_from_norm", "_host"):
            assert bits_equal(got[which + path], score), which + path
    return want


@pytest.mark.parametrize("name", list(CASES))
def test_norms_and_scores_match_the_numpy_statement(ctx, name):
    A = CASES[name]()
    n = A.shape[1]
    x, l, u = vectors(n, 7)
    dA = ctx.matrix(A)
    got = device_results(ctx, dA, x, l, u)
    dA.free()
    want = assert_matches_oracle(got, A, x, l, u)
    q, score = want["sumsq"], want["score"]
    if name == "long_column":
        assert np.diff(NO.stored_csc(A)[0])[1] == 9001
    if name == "extreme_values":
        assert q[5] == 0 and 0 < q[6] < 2.3e-308 and q[7] == np.inf and score[5] == 0.0
        assert np.count_nonzero(np.isinf(q)) > 10 and np.count_nonzero((q == 0) & (np.diff(NO.stored_csc(A)[0]) > 0)) >= 1
    if name in ("empties", "nnz0"):
        assert np.count_nonzero(q == 0) >= 40 and not np.any(np.signbit(score[q == 0]))
    if n > 100:                                              # the numerator cases are all there
        free = (l == -np.inf) & (u == np.inf)
        assert free.any() and (np.isinf(l) & ~free).any() and (np.isinf(u) & ~free).any()
        assert np.isnan(x[n // 2]) and (np.isnan(score[n // 2]) or q[n // 2] == 0)
        assert np.any(score < 0) or name == "nnz0"


@pytest.mark.parametrize("gname", ["g1", "g2"])
def test_golden_matrices_with_their_interior_point(ctx, gname, request):
    g = request.getfixturevalue(gname)
    A = csr_from(g, "A")
    x, l, u = np.asarray(g["x"], dtype=np.float64), np.asarray(g["l"], dtype=np.float64), np.asarray(g["u"], dtype=np.float64)
    dA = ctx.matrix(A)
    got = device_results(ctx, dA, x, l, u)
    dA.free()
    assert_matches_oracle(got, A, x, l, u, NO.column_sumsq_loop(A))


def test_norms_are_cached_on_the_matrix(ctx):
    A = random_n(257)
    dA = ctx.matrix(A)
    first = dA.column_norms()
    assert dA.column_norms() is first
    assert bits_equal(first.download(), NO.norm_score(A, *vectors(257, 1), "abs")["norm"])
    dA.free()
    assert first.ptr is None and dA._col_norms is None


def test_column_shard_is_accepted_and_row_shard_refused(ctx):
    from smart_crossover.hip import lib as sxl
    A = duplicates_unsorted()
    csc = sp.csr_matrix(A).tocsc()                           # stored order of the derived layout
    n = A.shape[1]
    x, l, u = vectors(n, 9)
    dC = ctx.column_shard(csc)
    got = device_results(ctx, dC, x, l, u)
    dC.free()
    assert_matches_oracle(got, A, x, l, u, NO.sumsq_from_csc(csc.indptr, csc.indices, csc.data, A.shape[0]))
    dR = ctx.row_shard(A)
    out = ctx.empty(n, np.float64)
    with pytest.raises(sxl.SxError, match="no CSC layout"):
        ctx.column_norms(dR, norm=out)
    with pytest.raises(sxl.SxError, match="no CSC layout"):
        ctx.score_norm(dR, ctx.to_device(x), None, None, "abs")
    # the C entry points return SX_ERR_INVALID, as K1 does for a row shard
    assert ctx._lib.sx_column_norms_dev(ctx.handle, dR.handle, None, out.ptr) == sxl.SX_ERR_INVALID
    assert ctx._lib.sx_score_norm(ctx.handle, dR.handle, x.ctypes.data, None, None, sxl.NORM_ABS, None,
                                  np.empty(n).ctypes.data) == sxl.SX_ERR_INVALID
    dR.free()


def test_package_indicator_and_device_ranking():
    """lp_methods.algorithms.get_norm_indicator / rank_by_norm_indicator: the oracle's bits, and K9's order -- descending
    indicator, equal keys by descending index, NaN first -- on an LP with identical columns (ties) and a NaN."""
    from smart_crossover.formats import GeneralLP
    from smart_crossover.hip.resident import resident_for
    from smart_crossover.lp_methods import algorithms as alg
    from _dist_worker_norm import problem
    lp, x = problem()
    x = x.copy()
    x[7] = np.nan
    for which in ("gap", "abs"):
        want = NO.norm_score(lp.A, x, lp.l, lp.u, which)["score"]
        assert np.isnan(want[7]) and np.count_nonzero(want == want[0]) > 100
        assert bits_equal(alg.get_norm_indicator(lp, x, which), want)
        order = NO.rank_desc(want)
        assert order[0] == 7
        got = alg.rank_by_norm_indicator(lp, x, numerator=which)
        assert got.dtype == np.int64 and np.array_equal(got, order)
        assert np.array_equal(alg.rank_by_norm_indicator(lp, x, 25, which), order[:25])
    res = resident_for(lp)
    assert res.A.column_norms() is res.A.column_norms()      # A was uploaded once, its norms computed once
    assert isinstance(lp, GeneralLP) and lp._sx_resident is res
    res.free()


def test_sharded_lp_without_a_process_group(tmp_path):
    """``ShardedLP(lp, dist=None)`` with the real kernels in a fresh child process (torch initialises HIP before
    the first library context): own block = all columns, same bits as the single-context call, same ranking."""
    out = tmp_path / "res.json"
    env = dict(os.environ, SX_DIST_OPS="hip", LOCAL_RANK="0", OMP_NUM_THREADS="2")
    p = subprocess.run([sys.executable, os.path.join(HERE, "_dist_worker_norm.py"), str(out)], env=env,
                       capture_output=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr).decode(errors="replace")[-3000:]
    res = json.loads(out.read_text())
    assert res["world"] == 1 and len(res["blocks"]) == 1
    for which in ("gap", "abs"):
        r = res[which]
        assert r["ind_bits_equal"] and r["single_context_bits_equal"]
        assert r["top_equal"] == [True, True, True] and r["ties_in_top"] >= 100
