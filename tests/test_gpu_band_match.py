"""GPU: two stages of the sparse crossover's set-up on the device (csrc/sx_band_match.hip) -- basic columns matched to
band rows (sx_band_match_dev) and the band assembled as triplets (sx_band_triplets_dev) -- against a plain restatement of
the host rule (csrc/sx_band_plan.h: match_columns_to_rows, walk_band) on numpy arrays, exactly; and the product path under
context option "band_setup" 0 and 1, bit for bit."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import scipy.sparse as sp

import workloads

pytestmark = pytest.mark.gpu
MATCH_MIN = 1e-6


@pytest.fixture(scope="module")
def ctx():
    from smart_crossover.hip import default_context
    return default_context()


def host_rule(A, is_basic, rowb, m1, prev_pos=None):
    """Seeds, then two rounds (each column's best entry; all entries of the losers): edges sorted by (-size, variable, band
    row), an edge is taken if both its ends are free."""
    A = sp.csc_matrix(A)
    m, n = A.shape
    bvar, placed = np.full(m1, -1, dtype=np.int64), np.zeros(n + m, dtype=np.uint8)
    for p, v in enumerate([] if prev_pos is None else prev_pos):
        if v >= 0 and is_basic[v] and not placed[v]:
            bvar[p], placed[v] = v, 1
    for i in np.flatnonzero(rowb >= 0):
        if bvar[rowb[i]] < 0 and is_basic[n + i] and not placed[n + i]:
            bvar[rowb[i]], placed[n + i] = n + i, 1
    for best_only in (True, False):
        edges = []
        for j in np.flatnonzero(is_basic[:n] & (placed[:n] == 0)):
            k = slice(A.indptr[j], A.indptr[j + 1])
            mine = [(-abs(a), int(j), int(rowb[i])) for i, a in zip(A.indices[k], A.data[k])
                    if rowb[i] >= 0 and bvar[rowb[i]] < 0 and abs(a) > MATCH_MIN]
            edges += [min(mine, key=lambda e: (e[0], e[2]))] if best_only and mine else ([] if best_only else mine)
        for _, j, ib in sorted(edges):
            if not placed[j] and bvar[ib] < 0:
                bvar[ib], placed[j] = j, 1
    return bvar, placed


def hand():   # tests/test_band_plan_cpu.py::test_hand_written_case_pins_the_greedy_order
    rows = [0, 1, 2, 3, 0, 2, 1, 2, 3, 4, 4, 3, 0, 1, 5, 5]
    cols = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7]
    vals = [2.0, 1.0, 1.0, 1.0, 3.0, 0.5, 1.0, 1.0, 1e-7, 0.5, 0.5, 0.25, 0.1, 0.1, 1.0, 1.0]
    basic = np.r_[np.ones(6), np.zeros(8)].astype(np.uint8)
    return sp.coo_matrix((vals, (rows, cols)), shape=(6, 8)), basic, np.arange(6, dtype=np.int32), 6, None


def random_small(seed, with_prev=False):
    """Up to 18 rows (some dense), 16 columns, entries from a four-value set (one below MATCH_MIN): ties everywhere."""
    rng = np.random.default_rng(seed)
    m, n = int(rng.integers(6, 19)), 16
    A = sp.random(m, n, density=0.3, random_state=int(seed), data_rvs=lambda k: rng.choice([0.5, 1.0, 2.0, 1e-7], k) * rng.choice([-1, 1], k))
    band = np.flatnonzero(rng.random(m) < 0.8)[:14]
    rowb = np.full(m, -1, dtype=np.int32)
    rowb[band] = rng.permutation(band.size)
    basic = (rng.random(n + m) < np.r_[np.full(n, 0.7), np.full(m, 0.25)]).astype(np.uint8)
    prev = None
    if with_prev and band.size >= 3:
        prev = np.full(band.size, -1, dtype=np.int64)
        cols = rng.permutation(n)
        basic[cols[0]], basic[cols[1]] = 1, 0
        prev[0], prev[1] = cols[0], cols[1]            # a kept variable, one that is no longer basic
        i = int(band[0] if rowb[band[0]] != 2 else band[1])   # a basic logical held on another position than its own row's
        basic[n + i] = 1
        prev[2] = n + i
    return A, basic, rowb, int(band.size), prev


def chain(N=40):
    """Column j waits for column j - 1: one mutual-best round per column (38 in a model on the CPU)."""
    e = [(0, 0, 1000.0)] + [t for j in range(1, N - 1) for t in ((0, j, 500.0 - j), (j, j, 2.0 * N - 2 * j), (j + 1, j, 2.0 * N - 2 * j - 1))]
    r, c, v = zip(*e)
    return sp.coo_matrix((v, (r, c)), shape=(N, N - 1)), np.r_[np.ones(N - 1), np.zeros(N)].astype(np.uint8), np.arange(N, dtype=np.int32), N, None


def one_dense_column(m=300):
    rng = np.random.default_rng(3)
    short = sp.random(m, m, density=2.5 / m, random_state=3, data_rvs=lambda k: rng.choice([0.5, 1.0, 2.0], k))
    A = sp.hstack([sp.csr_matrix(rng.choice([0.5, 1.0, 2.0], (m, 1))), short])
    return A, np.r_[np.ones(m + 1), np.zeros(m)].astype(np.uint8), rng.permutation(m).astype(np.int32), m, None


def empties(which):
    A = sp.csr_matrix(np.array([[1.0, 2.0, 0.0], [0.5, 0.0, 3.0], [0.0, 1.0, 1.0]]))
    basic = np.array([1, 1, 1, 0, 0, 0], dtype=np.uint8)
    if which == "m1=1":
        return A, basic, np.array([-1, 0, -1], dtype=np.int32), 1, None
    if which == "nothing basic":
        return A, np.zeros(6, dtype=np.uint8), np.arange(3, dtype=np.int32), 3, None
    return sp.csr_matrix(np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 1.0], [0.0, 1.0, 3.0]])), basic, np.array([-1, 0, 1], dtype=np.int32), 2, None


CASES = {"hand": hand, "chain": chain, "dense column": one_dense_column,
         **{f"random {s}": (lambda s=s: random_small(s)) for s in range(4)},
         **{f"prev_pos {s}": (lambda s=s: random_small(s, True)) for s in (10, 11, 12)},
         **{w: (lambda w=w: empties(w)) for w in ("m1=1", "nothing basic", "column outside the band")}}


def device_match(ctx, A, basic, rowb, m1, prev):
    dA = ctx.matrix(sp.csr_matrix(A))
    bvar, placed, rounds = ctx.band_match(dA, ctx.to_device(basic), ctx.to_device(rowb), m1, None if prev is None else ctx.to_device(prev))
    out = bvar.download(), placed.download(), rounds
    dA.free()
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_matching_is_the_host_rule(ctx, name):
    A, basic, rowb, m1, prev = CASES[name]()
    want_bvar, want_placed = host_rule(A, basic, rowb, m1, prev)
    bvar, placed, rounds = device_match(ctx, A, basic, rowb, m1, prev)
    print(name, "rounds", rounds, "matched", int((bvar >= 0).sum()), "of", m1)
    assert np.array_equal(bvar, want_bvar) and np.array_equal(placed, want_placed)
    if name == "hand":
        assert bvar.tolist() == [1, 2, 0, 4, 3, -1]
    if name.startswith("prev_pos"):
        assert bvar[0] == prev[0] and bvar[1] != prev[1] and bvar[2] == prev[2] and rowb[prev[2] - A.shape[1]] != 2
    if name == "chain":
        assert rounds > 8, "the chain has to take more rounds than one launch group holds"


def test_chain_by_direct_launches_and_by_graph_replay_agree(ctx):
    A, basic, rowb, m1, prev = chain()
    want = host_rule(A, basic, rowb, m1)
    try:
        ctx.set_option("graph", 0)
        eager = device_match(ctx, A, basic, rowb, m1, prev)
    finally:
        ctx.set_option("graph", 1)
    replay = device_match(ctx, A, basic, rowb, m1, prev)
    for got in (eager, replay):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == eager[2]


def staircase():
    inst = workloads.netlib_lp(800, 8000)
    m, n = inst.A.shape
    per_row = np.diff(inst.A.indptr)
    band = np.flatnonzero(per_row <= max(24, int(6.0 * inst.A.nnz / m)))
    rowb = np.full(m, -1, dtype=np.int32)
    rowb[band] = np.arange(band.size)
    basic = np.r_[(inst.x > inst.l + 1e-7) & (inst.x < inst.u - 1e-7), np.zeros(m, dtype=bool)].astype(np.uint8)
    return inst.A, basic, rowb, int(band.size), None


@pytest.mark.parametrize("make", [lambda: random_small(1), one_dense_column, staircase], ids=["random 1", "dense column", "netlib_lp(800, 8000)"])
def test_band_triplets_are_the_walk_of_the_matched_columns(ctx, make):
    A, basic, rowb, m1, prev = make()
    A = sp.csc_matrix(A)
    n = A.shape[1]
    bvar = host_rule(A, basic, rowb, m1, prev)[0]
    cut, npad = m1 // 2, 5                    # an epoch's positions: padding (-2) in the middle, as between two blocks
    bvar = np.r_[bvar[:cut], np.full(npad, -2), bvar[cut:]].astype(np.int64)
    rowb = np.where(rowb >= cut, rowb + npad, rowb).astype(np.int32)
    want = []
    for p, v in enumerate(bvar):
        k = slice(A.indptr[v], A.indptr[v + 1]) if 0 <= v < n else slice(0, 0)
        want += [(p, p, 1.0)] if not 0 <= v < n else [(p, int(rowb[i]), a) for i, a in zip(A.indices[k], A.data[k]) if rowb[i] >= 0]
    want.sort()
    dA = ctx.matrix(sp.csr_matrix(A))
    row, col, val, kl, ku = ctx.band_triplets(dA, ctx.to_device(bvar), ctx.to_device(rowb))
    row, col, val = row.download(), col.download(), val.download()
    dA.free()
    order = np.lexsort((row, col))
    assert list(zip(col[order].tolist(), row[order].tolist(), val[order].tolist())) == want
    assert (kl, ku) == (max(max(r - c, 0) for c, r, _ in want), max(max(c - r, 0) for c, r, _ in want))


@pytest.mark.parametrize("eta", [None, "16"], ids=["one epoch", "eta file of 16: several epochs, prev_pos in use"])
def test_product_path_is_the_same_with_the_set_up_on_either_side(ctx, monkeypatch, eta):
    if eta:
        monkeypatch.setenv("SX_BAND_EPOCH", eta)
    from smart_crossover.formats import GeneralLP
    from smart_crossover.lp_methods import algorithms as alg
    inst = workloads.netlib_lp(3000, 30000)
    with redirect_stdout(io.StringIO()):
        mgr = alg.get_perturb_problem(GeneralLP(inst.A, inst.b, inst.c, inst.l, inst.u, inst.sense), inst.x, inst.y, 1e-3, 1e-3, False)
    sub = mgr.lp_sub
    m, n = sub.A.shape
    dA = ctx.matrix(sub.A)
    put = lambda v, t=np.float64: ctx.to_device(np.ascontiguousarray(v, dtype=t))   # noqa: E731
    args = [put(sub.b), put(sub.c), put(sub.l), put(sub.u), put(np.asarray(sub.sense) == "<", np.uint8), put(mgr.get_subx(inst.x))]
    got = []
    try:
        for side in (0, 1):
            ctx.set_option("band_setup", side)
            out = ctx.empty(n, np.float64), ctx.empty(m, np.float64), ctx.empty(n, np.int8), ctx.empty(m, np.int8)
            res = ctx.crossover_band(dA, *args, 0, 1e-7, 1e-7, *out)
            got.append((int(res.status), int(res.iters), *[o.download() for o in out]))
    finally:
        ctx.set_option("band_setup", 0)
    dA.free()
    host, dev = got
    print("status", host[0], dev[0], "iterations", host[1], dev[1])
    assert host[0] == dev[0] == 0 and host[1] == dev[1] and (eta is None or host[1] > 16)
    assert np.array_equal(host[4], dev[4]) and np.array_equal(host[5], dev[5])
    assert np.array_equal(host[2].view(np.uint64), dev[2].view(np.uint64)), "x differs between host and device set-up"
