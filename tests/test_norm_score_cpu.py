"""CPU: the NumPy statement of the norm-scaled column indicator (tests/_norm_oracle.py), the no-GPU rule for its
package entry points, and ``ShardedLP.norm_indicator`` / ``top_columns`` rehearsed over gloo."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _norm_oracle as NO  # noqa: E402


def test_matvec_form_equals_the_left_to_right_loop():
    """300 x 701, magnitudes over 1e-8 .. 1e8, duplicates and unsorted inner indices kept: the csr_matvec form of the
    column sums has the bits of the explicit sequential loop (a pairwise sum would not)."""
    rng = np.random.default_rng(3)
    m, n, nnz = 300, 701, 9000
    rows, cols = rng.integers(0, m, nnz), rng.integers(0, n - 9, nnz)     # the last nine columns stay empty
    cols[:2000] = rng.integers(0, 12, 2000)                  # a few long columns
    vals = rng.choice([-1.0, 1.0], nnz) * 10.0 ** rng.uniform(-8, 8, nnz)
    order = np.argsort(rows, kind="stable")
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))])
    A = sp.csr_matrix((vals[order], cols[order], indptr), shape=(m, n))      # unsorted, with duplicates
    assert not A.has_sorted_indices and A.nnz == nnz
    q, q_loop = NO.column_sumsq(A), NO.column_sumsq_loop(A)
    assert np.array_equal(q.view(np.uint64), q_loop.view(np.uint64))
    assert np.count_nonzero(q == 0) > 0 and np.diff(NO.stored_csc(A)[0]).max() > 100
    # the statement is about the ORDER: the pairwise sum of the same squares differs somewhere
    indptr_c, _, data_c = NO.stored_csc(A)
    nonempty = np.flatnonzero(np.diff(indptr_c))
    pairwise = np.add.reduceat(data_c * data_c, indptr_c[nonempty])
    assert not np.array_equal(pairwise, q[nonempty])


def test_numerators_and_empty_columns():
    A = sp.csr_matrix(np.array([[3.0, 0.0, 1e200, 1.0], [4.0, 0.0, 0.0, 0.0]]))
    x = np.array([2.5, 7.0, 1.0, np.nan])
    l = np.array([0.0, 0.0, -np.inf, 0.0])
    u = np.array([4.0, 1.0, np.inf, 1.0])
    r = NO.norm_score(A, x, l, u, "gap")
    assert r["sumsq"].tolist()[:3] == [25.0, 0.0, np.inf] and r["norm"][0] == 5.0
    assert r["score"][0] == 1.5 / 5.0 and r["score"][1] == 0.0 and r["score"][2] == 0.0 and np.isnan(r["score"][3])
    assert NO.norm_score(A, -x, l, u, "abs")["score"][0] == 0.5
    assert NO.norm_score(A, np.array([5.0, 0, 0, 0]), l, u, "gap")["score"][0] == -0.2       # outside the bounds
    assert NO.rank_desc(np.array([1.0, np.nan, 1.0, 2.0])).tolist() == [1, 3, 2, 0]


def test_no_gpu_means_loud_failure_for_the_norm_indicator():
    """Without a GPU the package entry points raise; nothing is computed on the CPU."""
    from smart_crossover.hip import lib as sxl
    if sxl.device_count() > 0:
        pytest.skip("a GPU is present")
    from smart_crossover.formats import GeneralLP
    from smart_crossover.lp_methods import algorithms as alg
    lp = GeneralLP(sp.identity(3, format="csr"), np.ones(3), np.ones(3), np.zeros(3), np.ones(3), np.full(3, "="))
    for fn in (alg.get_norm_indicator, alg.rank_by_norm_indicator):
        with pytest.raises((sxl.SxLibraryError, sxl.SxError)):
            fn(lp, np.ones(3))


def test_invalid_error_is_an_sxerror_and_a_valueerror():
    from smart_crossover.hip import lib as sxl
    assert issubclass(sxl.SxInvalidError, sxl.SxError) and issubclass(sxl.SxInvalidError, ValueError)
    sxl.check_sx(sxl.SX_OK)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_norm_indicator_over_gloo(tmp_path, world):
    """Own column block only, no communication: the concatenated per-rank indicators have the bits of the
    single-process oracle, and the merged per-rank top-k lists are the single-process ranking -- on an LP whose
    identical columns sit on both sides of every rank boundary, so that runs of ties cross it."""
    from test_dist_gloo import run_workers
    res = run_workers("_dist_worker_norm.py", tmp_path / "res.json", world)
    assert res["world"] == world and len(res["blocks"]) == world
    for start, stop in res["blocks"]:
        assert stop - start >= 6                             # every block holds several of the identical columns
    for which in ("gap", "abs"):
        r = res[which]
        assert r["ind_bits_equal"]
        assert r["top_equal"] == [True, True, True]
        assert r["ties_in_top"] >= 100
