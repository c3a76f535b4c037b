"""NumPy statement of the norm-scaled column indicator (include/sxhip.h, K17) -- TEST INFRASTRUCTURE.

This restates no reference code: the reference has no |x_j| / ||A_j|| score.  It is the
arithmetic contract of sx_column_norms_dev / sx_score_norm_dev written down once more, independently of the kernel:

    q_j     = (((+0.0 + a_k0*a_k0) + a_k1*a_k1) + ...)     entries of column j in the library's stored order
    norm_j  = np.sqrt(q_j)
    num_j   = |x_j|                                        "abs"
    num_j   = np.minimum(x_j - l_j, u_j - x_j), |x_j| where l_j = -inf and u_j = +inf      "gap"
    score_j = +0.0 where q_j == 0, else num_j / norm_j

The column sums are one scipy ``csr_matvec`` of the squared values against a vector of ones: a sequential loop over
the stored entries of every column, every product (s * 1.0, exact) and every sum rounded on its own.  The arrays are
neither summed, sorted nor de-duplicated on the way.  (``np.add.reduceat`` would NOT do: it sums pairwise.)"""
import numpy as np
import scipy.sparse as sp


def stored_csc(A):
    """(indptr, indices, data) of the library's derived column layout: the stable transposition of the CSR arrays
    (scipy's csr_tocsc), duplicates and unsorted inner indices kept as stored."""
    csc = sp.csr_matrix(A).tocsc()
    return csc.indptr, csc.indices, csc.data


def sumsq_from_csc(indptr, indices, data, m):
    """q of the columns of an explicit CSC layout (a column shard is handed over in this form)."""
    n = len(indptr) - 1
    d = np.asarray(data, dtype=np.float64)
    with np.errstate(all="ignore"):
        sq = sp.csr_matrix((d * d, indices, indptr), shape=(n, m))
        return np.asarray(sq @ np.ones(m), dtype=np.float64)


def column_sumsq(A):
    indptr, indices, data = stored_csc(A)
    return sumsq_from_csc(indptr, indices, data, sp.csr_matrix(A).shape[0])


def column_sumsq_loop(A):
    """The same sums by the explicit left-to-right Python loop (what the matvec is checked against)."""
    indptr, _, data = stored_csc(A)
    q = np.zeros(len(indptr) - 1)
    with np.errstate(all="ignore"):
        for j in range(q.size):
            s = np.float64(0.0)
            for k in range(indptr[j], indptr[j + 1]):
                s = s + data[k] * data[k]
            q[j] = s
    return q


def numerator(x, l, u, which):
    x = np.asarray(x, dtype=np.float64)
    if which == "abs":
        return np.abs(x)
    assert which == "gap"
    with np.errstate(all="ignore"):
        gap = np.minimum(x - l, u - x)
    free = (l == -np.inf) & (u == np.inf)
    return np.where(free, np.abs(x), gap)


def score_from_sumsq(q, x, l, u, which):
    with np.errstate(all="ignore"):
        ratio = numerator(x, l, u, which) / np.sqrt(q)
    return np.where(q == 0, 0.0, ratio)


def norm_score(A, x, l, u, which):
    """dict(sumsq, norm, score) for the columns of A."""
    q = column_sumsq(A)
    with np.errstate(all="ignore"):
        nrm = np.sqrt(q)
    return dict(sumsq=q, norm=nrm, score=score_from_sumsq(q, x, l, u, which))


def rank_desc(score):
    """The library's ranking rule (K9): descending key, equal keys by descending index, NaN first."""
    return np.argsort(score, kind="stable")[::-1]
