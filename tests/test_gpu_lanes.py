"""GPU parity of the lane-major column walk (csrc/sx_lanes.h): K1 and K10 over the lane-major copy of the columns
against the oracle, bit for bit -- s_d, column codes, reduced costs, the price record's minimum and argmin and the
violation count -- under the "lanes" and "window" options, on matrices that are and are not eligible for the copy.

The matrices are handed over as column shards (CSC as stored), and the oracle sums a column in stored order from +0.0
(scipy's csr_matvec on the transposed view), so unsorted and duplicate row indices are part of the comparison."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import bits_equal
from oracle import lp_path as L
from oracle import net_path as N
import workloads

pytestmark = pytest.mark.gpu

M_RAGGED = 8192


@pytest.fixture(scope="module")
def ctx():
    from smart_crossover.hip import Context
    c = Context(0)
    yield c
    c.close()


def lane_layout(indptr):
    """(tiles, longest column, slots) of the lane-major copy, from the rules of csrc/sx_tiles.hip (a tile ends at every
    256th column and wherever the entry offset inside that block of 256 crosses a multiple of the budget) and of
    csrc/sx_lanes.h (a tile of ncol columns, longest L rounded up to even, takes L x (ncol rounded up to even) slots)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n, nnz = indptr.size - 1, int(indptr[-1])
    budget = 8192
    while budget > 1024 and nnz // budget < 2048:
        budget //= 2
    s = np.arange(n)
    origin = indptr[s - s % 256]
    cut = (s % 256 == 0)
    cut[1:] |= ((indptr[1:n] - origin[1:]) // budget) != ((indptr[0:n - 1] - origin[1:]) // budget)
    starts = np.append(np.flatnonzero(cut), n)
    lens = np.diff(indptr)
    slots, longest = 0, 0
    for a, b in zip(starts[:-1], starts[1:]):
        lmax = int(lens[a:b].max())
        longest = max(longest, lmax)
        slots += ((lmax + 1) & ~1) * ((b - a + 1) & ~1)
    return starts.size - 1, longest, slots


def eligible(indptr):
    _, longest, slots = lane_layout(indptr)
    return longest <= 64 and 8 * slots <= 9 * int(indptr[-1])


def ragged_columns(n, seed=3, long_column=None):
    """m = 8,192 rows, n columns in CSC as stored.  Most lengths are 12, one in seven is drawn from 0..12 (a flat draw
    from 0..12 for every column would pad each tile to twice its entries: not eligible); columns 5 and n - 1 are empty;
    when n > 290, columns 256..289 -- the head of a block of 256, so that the tile cuts fall between them and the short
    columns -- hold 2,048 entries in columns of 60..63, exactly one of 63.  Row indices are drawn unsorted inside a
    3,000-row band that moves with the column, 5 % anywhere; every seventh column repeats its first index.  Column 40
    has five entries on rows where y is -0.0 and positive values: all its products are -0.0.
    ``long_column``: (column, length) replaces that column's entries -- 5,000 make the matrix ineligible."""
    rng = np.random.default_rng(seed)
    m = M_RAGGED
    lens = np.where(rng.random(n) < 6 / 7, 12, rng.integers(0, 13, n))
    lens[[5, n - 1]] = 0
    lens[40] = 5
    if n > 290:
        lens[256:290] = [63] + [61] * 5 + [60] * 28
    if long_column:
        lens[long_column[0]] = long_column[1]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.repeat(np.arange(n), lens)
    band_lo = (col * (m - 3000)) // n
    rows = band_lo + rng.integers(0, 3000, col.size)
    anywhere = rng.random(col.size) < 0.05
    rows[anywhere] = rng.integers(0, m, int(anywhere.sum()))
    for j in range(0, n, 7):
        if lens[j] >= 2:
            rows[indptr[j] + 1] = rows[indptr[j]]
    vals = rng.standard_normal(col.size)
    y = rng.standard_normal(m)
    special = rng.permutation(m)[:160]
    y[special[:40]] = np.inf
    y[special[40:80]] = -np.inf
    y[special[80:120]] = np.nan
    y[special[120:160]] = -0.0
    rows[indptr[40]:indptr[41]] = special[120:125]
    vals[indptr[40]:indptr[41]] = np.abs(vals[indptr[40]:indptr[41]]) + 0.5
    A = sp.csc_matrix((vals, rows.astype(np.int32), indptr), shape=(m, n))
    c = rng.standard_normal(n)
    c[40] = -0.0
    vec = {"y": y, "c": c, "x": rng.standard_normal(n), "l": np.where(rng.random(n) < 0.2, -np.inf, 0.0),
           "u": np.where(rng.random(n) < 0.5, np.inf, 2.0)}
    return A, vec


def check_settings(ctx, A, vec, settings, expect_lanes):
    """K1 and K10 on the column shard A under every (lanes, window) of ``settings`` against the oracle;
    expect_lanes(lanes, window) says whether the handle must report a lane-major copy under that setting."""
    n = A.shape[1]
    want_sd = L.dual_slack(A, vec["c"], vec["y"])
    want_code = L.column_codes(vec["x"], vec["l"], vec["u"], want_sd, L.GAMMA0)
    vb = np.random.default_rng(5).integers(-2, 1, n).astype(np.int8)
    want_rc = N.mcf_reduced_cost(A, vec["c"], vec["y"], vb.astype(int))
    finite = want_rc[~np.isnan(want_rc)]
    want_min = finite.min()
    want_arg = int(np.flatnonzero(want_rc == want_min)[0])
    want_bad = int(np.count_nonzero(~(want_rc >= -1e-6)))
    tiles, _, slots = lane_layout(A.indptr)
    dC = ctx.column_shard(A)
    d = {k: ctx.to_device(v) for k, v in vec.items()}
    dvb = ctx.to_device(vb)
    try:
        for lanes, window in settings:
            key = (lanes, window)
            ctx.set_option("lanes", lanes)
            ctx.set_option("window", window)
            s_d, code, rc = ctx.empty(n, np.float64), ctx.empty(n, np.uint8), ctx.empty(n, np.float64)
            ctx.score_columns(dC, d["y"], d["c"], d["x"], d["l"], d["u"], L.GAMMA0, s_d, code)
            res = ctx.price(dC, d["y"], d["c"], dvb, 1e-6, rc)
            assert bits_equal(s_d.download(), want_sd), key
            assert np.array_equal(code.download(), want_code), key
            assert bits_equal(rc.download(), want_rc), key
            mn, am, bad = ctx.read_price(res)
            assert mn == want_min and am == want_arg and bad == want_bad, key
            info = dC.lanes()
            if expect_lanes(lanes, window):
                assert info == dict(tiles=tiles, slots=slots, bytes=256 * tiles + 12 * slots), key
            else:
                assert info is None, key
    finally:
        ctx.set_option("lanes", -1)
        ctx.set_option("window", -1)
        dC.free()
    return want_sd, want_rc


def test_lanes_staircase_every_setting(ctx):
    """The staircase shard of the bench at 40,000 x 60,000, 8 entries per column (nothing padded); the linking-row entry
    of every column and half of the next-stage entries lie outside the window and are served from global memory.  469
    tiles (the tile budget of a matrix this small is 1,024 entries), so the last run of 4 holds one tile.  The auto rule
    of the window says yes on this matrix."""
    sh = workloads.lp_shard(0, 1, m=40_000, n_block=60_000, k=8, structure="staircase", window=4096)
    A = sp.csc_matrix(sh.col_block)
    tiles, longest, slots = lane_layout(A.indptr)
    assert tiles % 4 != 0 and longest == 8 and slots == A.nnz
    vec = {"y": sh.y, "c": sh.c, "x": sh.x[:A.shape[1]], "l": sh.l, "u": sh.u}
    settings = [(ln, w) for ln in (0, 1, -1) for w in (0, 4, -1)]
    check_settings(ctx, A, vec, settings, lambda ln, w: ln != 0 and w != 0)


def test_lanes_ragged_eligible(ctx):
    """Ragged but eligible (see ragged_columns): empty columns, one of 63 entries, unsorted and duplicate indices, rows
    outside the window, +-inf, NaN and -0.0 in y, a column of -0.0 products under a -0.0 cost, NaN reduced costs that
    must not become the minimum.  A padded slot that was added would show wherever its row holds inf or NaN."""
    A, vec = ragged_columns(1000)
    lens = np.diff(A.indptr)
    assert eligible(A.indptr) and lens.max() == 63 and np.count_nonzero(lens == 63) == 1 and (lens == 0).sum() >= 2
    want_sd, want_rc = check_settings(ctx, A, vec, [(0, 4), (1, 4), (-1, 4), (1, 0), (1, 8), (1, 1)],
                                      lambda ln, w: ln != 0 and w != 0)
    assert np.signbit(want_sd[40]) and want_sd[40] == 0.0
    assert np.isnan(want_rc).any() and np.isinf(want_rc).any()


def test_lanes_not_eligible_falls_back(ctx):
    """One column of 5,000 entries: no copy is built under "lanes" = 1, the staged walk gives the oracle's bits."""
    A, vec = ragged_columns(1000, long_column=(500, 5000))
    assert not eligible(A.indptr)
    check_settings(ctx, A, vec, [(1, 4), (-1, 4), (0, 4)], lambda ln, w: False)


def test_lanes_fewer_tiles_than_one_run(ctx):
    """300 columns in six tiles: one full and one partial run of 4, less than one run of 8; the last tile has 44 columns."""
    A, vec = ragged_columns(300)
    assert eligible(A.indptr) and lane_layout(A.indptr)[0] < 8
    check_settings(ctx, A, vec, [(-1, 4), (1, 4), (1, 8), (0, 4)], lambda ln, w: ln != 0)


def test_lanes_auto_waits_for_the_second_walk(ctx):
    """Option -1 builds no copy for a matrix that has not been walked, and none during its first K1; 1 builds at once."""
    A, vec = ragged_columns(300)
    n = A.shape[1]
    d = {k: ctx.to_device(v) for k, v in vec.items()}
    s_d, code = ctx.empty(n, np.float64), ctx.empty(n, np.uint8)
    ctx.set_option("window", 4)
    try:
        dC = ctx.column_shard(A)
        assert dC.lanes() is None
        ctx.score_columns(dC, d["y"], d["c"], d["x"], d["l"], d["u"], L.GAMMA0, s_d, code)
        assert bits_equal(s_d.download(), L.dual_slack(A, vec["c"], vec["y"]))
        assert dC.lanes() is not None               # due now: the matrix has been walked once
        dC.free()
        dC = ctx.column_shard(A)
        ctx.set_option("lanes", 1)
        assert dC.lanes() is not None
        dC.free()
    finally:
        ctx.set_option("lanes", -1)
        ctx.set_option("window", -1)
