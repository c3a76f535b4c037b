"""CPU: the side arrays of the row-block layout's staged long rows (tools/rb_layout.py stage_long, the numpy
statement of csrc/sx_rowblock.h): the pieces of the column-ordered list, the rank of every entry inside its piece
and the place where the walk finds the product of a long slot.  Products taken through them are, bit for bit, the
products of the layout's own entries, and the row sums finished from them are the oracle's."""
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

PARAMS = dict(R=512, cwin=4096, chunk=2048, dense_min=512, budget=96 * 512, merge_max=32768)


def staircase(m, nb, window, seed=5):
    sh = workloads.lp_shard(0, 1, m=m, n_block=nb, k=8, seed=seed, structure="staircase", window=window)
    return sh.row_block, sh.x, sh.b


def hand_made(seed=11):
    """Five long rows of 600 entries (fewer than one piece) with duplicate columns, among short rows; columns
    beyond 7000 are empty."""
    rng = np.random.default_rng(seed)
    m, n = 900, 9_000
    lens = rng.integers(0, 9, size=m)
    lens[100:105] = 600                                                 # consecutive: one super-tile
    cols = [np.sort(rng.integers(0, 7_000, size=k)) for k in lens]      # with replacement: duplicates
    A = sp.csr_matrix((rng.uniform(-1, 1, int(lens.sum())), np.concatenate(cols), np.concatenate([[0], np.cumsum(lens)])),
                      shape=(m, n))
    return A, rng.standard_normal(n), rng.standard_normal(m)


CASES = {"staircase_3000": (lambda: staircase(3_000, 30_000, 64), 8192),
         "staircase_20000": (lambda: staircase(20_000, 200_000, 512), 8192),
         "hand_made": (hand_made, 8192),
         "hand_made_small_pieces": (hand_made, 256)}


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    make, piece = CASES[request.param]
    A, x, b = make()
    lay = RB.build(A, **PARAMS)
    return A, x, b, lay, RB.stage_long(lay, piece), piece


def test_lperm_is_a_bijection_in_every_piece(case):
    A, x, b, lay, S, piece = case
    nl = S["nl"]
    assert nl > 0 and S["lperm"].dtype == np.uint16
    assert np.all(np.diff(S["lcol"].astype(np.int64)) >= 0)               # the list is in column order
    for base in range(0, nl, piece):
        got = np.sort(S["lperm"][base:base + piece].astype(np.int64))
        assert np.array_equal(got, np.arange(got.size)), base
    if piece == 8192 and nl > 8192:
        assert nl % piece != 0                                            # a partial last piece is among the cases


def test_lsrc_points_at_piece_base_plus_rank(case):
    A, x, b, lay, S, piece = case
    i = np.arange(S["nl"], dtype=np.int64)
    assert np.array_equal(S["lsrc"][S["le"]].astype(np.int64), (i // piece) * piece + S["lperm"])
    # ascending slots inside a piece get ascending ranks: the walk reads runs, and equal columns keep stored order
    for base in range(0, S["nl"], piece):
        sl, rk = S["le"][base:base + piece], S["lperm"][base:base + piece].astype(np.int64)
        assert np.all(np.diff(rk[np.argsort(sl, kind="stable")]) == 1)
    assert np.unique(S["le"]).size == S["nl"] and S["le"].max() < S["nls"]  # distinct long slots


def staged_products(S, x, piece):
    """What the pre-pass leaves in lprod: every piece's products at their ranks."""
    lprod = np.full(S["nl"] + 8, np.nan)
    i = np.arange(S["nl"], dtype=np.int64)
    lprod[(i // piece) * piece + S["lperm"]] = S["lval"] * x[S["lcol"]]
    return lprod


def test_products_through_lperm_and_lsrc_are_the_layouts_own(case):
    A, x, b, lay, S, piece = case
    lprod = staged_products(S, x, piece)
    live = np.sort(S["le"])                                               # long slots that hold an entry
    slot = S["lslot"][live]
    want = lay["val"][slot] * x[lay["idx"][slot]]
    assert bits_equal(lprod[S["lsrc"][live]], want)
    assert not np.isnan(lprod[:S["nl"]]).any()                            # every place of every piece was written


def test_row_sums_finished_from_the_staged_products_equal_the_oracle(case):
    A, x, b, lay, S, piece = case
    lprod = staged_products(S, x, piece)
    prod = lay["val"] * x[lay["idx"]]                                     # per slot; the long slots are replaced
    live = np.sort(S["le"])
    prod[S["lslot"][live]] = lprod[S["lsrc"][live]]
    # sequential sums per row in the order the walk adds: chunk after chunk, inside a chunk by stored order.
    # A CSR matrix of the products times a vector of ones adds exactly that way (a product times 1.0 is itself).
    ch, st, rs = lay["chunks"], lay["st"], lay["rowstart"]
    rows, slots = [], []
    for s in st:
        for k in range(s["chunk0"], s["chunk0"] + s["nchunks"]):
            c = ch[k]
            lo = np.maximum(rs[c["cell"], :s["nrows"]].astype(np.int64), c["base"])
            hi = np.minimum(rs[c["cell"], 1:s["nrows"] + 1].astype(np.int64), c["base"] + c["ne"])
            cnt = np.maximum(hi - lo, 0)
            r = np.repeat(np.arange(s["nrows"], dtype=np.int64), cnt)
            first = np.repeat(lo, cnt)
            within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            rows.append(s["row0"] + r)
            slots.append(int(c["e0"]) - int(c["base"]) + first + within)
    rows, slots = np.concatenate(rows), np.concatenate(slots)
    assert slots.size == A.nnz
    order = np.argsort(rows, kind="stable")                               # walk order survives inside a row
    m = A.shape[0]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))])
    P = sp.csr_matrix((prod[slots[order]], np.zeros(slots.size, dtype=np.int32), indptr), shape=(m, 1))
    sums = P @ np.ones(1)
    assert bits_equal(b - sums, L.primal_slack(A, b, x))


def test_a_layout_without_long_rows_has_no_staged_arrays():
    rng = np.random.default_rng(3)
    m, n, k = 1_500, 8_000, 10
    cols = np.sort(rng.integers(0, n, size=(m, k)), axis=1)
    A = sp.csr_matrix((rng.uniform(-1, 1, m * k), cols.ravel(), np.arange(m + 1) * k), shape=(m, n))
    S = RB.stage_long(RB.build(A, **PARAMS))
    assert S["nl"] == 0 and S["nls"] == 0 and not S["staged"].any() and S["lsrc"].size == 8
