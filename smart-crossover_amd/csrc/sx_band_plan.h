// Host set-up of the sparse crossover (K16s, sx_crossover_band.hip): everything between "here is an LP and a basic set"
// and "here are the triplets and index arrays the device factors" -- row classes and row order, the first basic set,
// columns matched to band rows, the block geometry of an epoch, band / border triplets and the bookkeeping after the two
// LUs.  Plain C++ over std::vector: no HIP, no error text (a failure is a return code plus the numbers the driver's message
// needs), nothing captured -- arguments in, results out.  The driver owns every device call between these stages; a
// device-side set-up would replace this header and nothing else.  tests/native/band_plan_check.cpp runs it under the host
// sanitizers.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

namespace sx_plan {

constexpr int64_t MAX_NB = 16384;      // rows of the Schur complement the dense LU takes
constexpr int32_t CM_TRIGGER = 600;    // a natural order with a taller column than this is tried in Cuthill-McKee order
constexpr double MATCH_MIN = 1e-6;     // smallest |entry| a column may sit on
constexpr double MARGIN = 1e-7;        // relative distance from a bound that makes a variable a candidate for the basis

// columns of A on the host (views: the driver owns the vectors)
struct Csc {
    int64_t m = 0, n = 0;
    const int64_t *ptr = nullptr;
    const int32_t *idx = nullptr;
    const double *val = nullptr;
};

// rows of a sparse matrix from (row, index, value) triplets (counting sort, stable); `list` != nullptr: only the rows
// that hold an entry, listed in ascending order
struct HostRows {
    std::vector<int64_t> ptr;
    std::vector<int32_t> idx, list;
    std::vector<double> val;
};
inline void rows_from_triplets(int64_t nrows, const std::vector<int32_t> &row, const std::vector<int32_t> &idx, const std::vector<double> &val,
                               bool compact, HostRows &out) {
    std::vector<int64_t> cnt(static_cast<size_t>(nrows) + 1, 0);
    for (int32_t r : row) ++cnt[static_cast<size_t>(r) + 1];
    for (int64_t r = 0; r < nrows; ++r) cnt[r + 1] += cnt[r];
    out.idx.assign(row.size(), 0);
    out.val.assign(row.size(), 0.0);
    std::vector<int64_t> at(cnt.begin(), cnt.end() - 1);
    for (size_t e = 0; e < row.size(); ++e) {
        const int64_t o = at[row[e]]++;
        out.idx[o] = idx[e];
        out.val[o] = val[e];
    }
    out.ptr.clear();
    out.list.clear();
    if (!compact) {
        out.ptr = cnt;
        return;
    }
    out.ptr.push_back(0);
    for (int64_t r = 0; r < nrows; ++r)
        if (cnt[r + 1] > cnt[r]) {
            out.list.push_back(static_cast<int32_t>(r));
            out.ptr.push_back(cnt[r + 1]);
        }
}

// ---------------------------------------------------------------------------------------------- rows: classes, order
// A row with more entries than this is DENSE (a linking row): it goes to the border, the others form the band.  The probe
// shortcut of the driver asks the device the same question with the same number.
inline int64_t dense_threshold(int64_t nnz, int64_t m) {
    const double avg_row = static_cast<double>(nnz) / static_cast<double>(m);
    return std::max<int64_t>(24, static_cast<int64_t>(6.0 * avg_row));
}

// The rows of the LP once per call: band rows in their order (natural, or Cuthill-McKee: order_band_rows), dense rows,
// and the two maps row -> band position (-1: dense) and row -> position in [band rows, dense rows].
struct RowPlan {
    std::vector<int32_t> rows_band, rows_dense, rowb, eqidx;
};
// rptr: [m + 1] row pointers of A.  Fills rows_band (natural order) and rows_dense; finish_row_plan fills the maps.
inline void classify_rows(int64_t m, const int64_t *rptr, int64_t dense_thr, RowPlan &out) {
    out.rows_band.clear();
    out.rows_dense.clear();
    for (int64_t i = 0; i < m; ++i) {
        if (rptr[i + 1] - rptr[i] > dense_thr) out.rows_dense.push_back(static_cast<int32_t>(i));
        else out.rows_band.push_back(static_cast<int32_t>(i));
    }
}
// rows spanned by the tallest column of A when the band rows are taken in `order` (rows not in it do not count)
inline int32_t tallest(const Csc &A, const std::vector<int32_t> &order) {
    std::vector<int32_t> where(static_cast<size_t>(A.m), -1);
    for (size_t k = 0; k < order.size(); ++k) where[order[k]] = static_cast<int32_t>(k);
    int32_t worst = 0;
    for (int64_t j = 0; j < A.n; ++j) {
        int32_t lo = INT32_MAX, hi = -1;
        for (int64_t k = A.ptr[j]; k < A.ptr[j + 1]; ++k) {
            const int32_t ib = where[A.idx[k]];
            if (ib >= 0) {
                lo = std::min(lo, ib);
                hi = std::max(hi, ib);
            }
        }
        if (hi >= 0) worst = std::max(worst, hi - lo);
    }
    return worst;
}
// The order of the band rows.  Natural order first (staged models are written stage after stage); when
// that leaves some column taller than a band can be, a Cuthill-McKee order of the rows (breadth first over
// "shares a column with", from a far end found by one extra sweep) -- rows of a model that was shuffled, or
// written variable by variable, fall back into stages.
// rptr / ridx: rows of A; nnz: its entries.  Returns false when the sweeps did not reach every band row (out is not an
// order then); the caller compares tallest(out) with tallest(rows_band) and takes the shorter.
inline bool cuthill_mckee_order(const Csc &A, const int64_t *rptr, const int32_t *ridx, int64_t nnz, const std::vector<int32_t> &rows_band,
                                std::vector<int32_t> &out) {
    const int64_t m1 = static_cast<int64_t>(rows_band.size());
    if (m1 == 0) return false;
    std::vector<uint8_t> is_band(static_cast<size_t>(A.m), 0);
    for (int32_t r : rows_band) is_band[r] = 1;
    const int64_t col_cap = std::max<int64_t>(64, static_cast<int64_t>(16.0 * static_cast<double>(nnz) / static_cast<double>(A.n)));
    auto sweep = [&](int32_t start, std::vector<int32_t> &order) { // breadth first over all components, `start` first
        order.clear();
        std::vector<uint8_t> seen(static_cast<size_t>(A.m), 0), used(static_cast<size_t>(A.n), 0);
        size_t next_seed = 0;
        int32_t seed = start;
        while (static_cast<int64_t>(order.size()) < m1) {
            if (seed < 0) {
                while (next_seed < rows_band.size() && seen[rows_band[next_seed]]) ++next_seed;
                if (next_seed >= rows_band.size()) break;
                seed = rows_band[next_seed];
            }
            size_t head_q = order.size();
            seen[seed] = 1;
            order.push_back(seed);
            for (; head_q < order.size(); ++head_q) {
                const int32_t i = order[head_q];
                for (int64_t k = rptr[i]; k < rptr[i + 1]; ++k) {
                    const int32_t j = ridx[k];
                    if (used[j]) continue;
                    used[j] = 1;
                    if (A.ptr[j + 1] - A.ptr[j] > col_cap) continue; // a column that touches everything orders nothing
                    for (int64_t q = A.ptr[j]; q < A.ptr[j + 1]; ++q) {
                        const int32_t i2 = A.idx[q];
                        if (is_band[i2] && !seen[i2]) {
                            seen[i2] = 1;
                            order.push_back(i2);
                        }
                    }
                }
            }
            seed = -1;
        }
    };
    std::vector<int32_t> o1;
    sweep(rows_band[0], o1);
    sweep(o1.empty() ? rows_band[0] : o1.back(), out); // from the far end of the first sweep
    return static_cast<int64_t>(out.size()) == m1;
}
// rows_band (in its final order) and rows_dense -> rowb, eqidx
inline void finish_row_plan(int64_t m, RowPlan &rp) {
    const int64_t m1 = static_cast<int64_t>(rp.rows_band.size()), ndr = static_cast<int64_t>(rp.rows_dense.size());
    rp.rowb.assign(static_cast<size_t>(m), -1);
    rp.eqidx.assign(static_cast<size_t>(m), 0);
    for (int64_t k = 0; k < m1; ++k) {
        rp.rowb[rp.rows_band[k]] = static_cast<int32_t>(k);
        rp.eqidx[rp.rows_band[k]] = static_cast<int32_t>(k);
    }
    for (int64_t k = 0; k < ndr; ++k) rp.eqidx[rp.rows_dense[k]] = static_cast<int32_t>(m1 + k);
}

// ---------------------------------------------------------------------------------------------- the basic set
// The basis bookkeeping that survives epochs.  Variables: [0, n) columns of A, n + i the logical of row i.
struct BasisState {
    std::vector<uint8_t> is_basic; // [n + m] the variables the next factorisation has to hold
    std::vector<int32_t> tracked;  // columns of the tableau that are not basic
    std::vector<int8_t> atup;      // [n + m] a non-basic column rests at its upper bound
    std::vector<int8_t> vstat;     // [n + m] 0 non-basic at a bound, 1 basic, 2 tracked (3: tracked and superbasic, at the end)
    std::vector<double> xlog;      // [m] values of tracked logicals
    std::vector<int64_t> prev_pos; // band position -> the variable that sat there and never moved
    std::vector<double> margin;    // of the first guess (empty for a given basis): the border takes its columns in this order
    std::vector<double> hx;        // [n] the point
    void init(int64_t n, int64_t m) {
        is_basic.assign(static_cast<size_t>(n + m), 0);
        tracked.clear();
        atup.assign(static_cast<size_t>(n + m), 0);
        vstat.assign(static_cast<size_t>(n + m), 0);
        xlog.assign(static_cast<size_t>(m), 0.0);
        prev_pos.clear();
        margin.clear();
    }
};
// THE order by margin: the surest variable first, ties by variable
struct MarginOrder {
    const std::vector<double> &margin;
    bool operator()(int64_t a, int64_t bb) const { return margin[a] > margin[bb] || (margin[a] == margin[bb] && a < bb); }
};
// a given basis: codes as in output.py (0 basic, -1 at lower, -2 at upper, -3 superbasic at x_start); a non-basic column
// is moved to the bound its code names (the other one, then 0, when that one is infinite).  vb [n], cb [m], lo / up [n].
inline void basic_set_from_codes(int64_t n, int64_t m, const int8_t *vb, const int8_t *cb, const double *lo, const double *up, BasisState &bs) {
    for (int64_t j = 0; j < n; ++j) {
        const int code = vb[j];
        if (code == 0) bs.is_basic[j] = 1;
        else if (code == -3) bs.tracked.push_back(static_cast<int32_t>(j));
        else {
            double v = code == -2 ? up[j] : lo[j];
            if (std::isinf(v)) v = code == -2 ? lo[j] : up[j];
            if (std::isinf(v)) v = 0.0;
            bs.hx[j] = v;
        }
    }
    for (int64_t i = 0; i < m; ++i)
        if (cb[i] == 0) bs.is_basic[n + i] = 1;
}
// a guess from the margins of the point bs.hx (within its bounds) and its slacks b - A x: every variable off its bounds is
// a candidate; the m candidates with the largest margins may sit in the basis, the others start superbasic.  Returns the
// number of candidates.
inline size_t basic_set_from_margins(int64_t n, int64_t m, const double *lo, const double *up, const double *rhs, const uint8_t *row_is_lt,
                                     const double *slack, BasisState &bs) {
    const std::vector<double> &hx = bs.hx;
    bs.margin.assign(static_cast<size_t>(n + m), -1.0);
    std::vector<int64_t> cand;
    for (int64_t j = 0; j < n; ++j) {
        const double mg = std::min(hx[j] - lo[j], up[j] - hx[j]);
        if (std::isinf(lo[j]) && std::isinf(up[j])) bs.margin[j] = 1e300;
        else if (mg > MARGIN * (1.0 + std::fabs(hx[j]))) bs.margin[j] = mg;
        if (bs.margin[j] > 0) cand.push_back(j);
    }
    for (int64_t i = 0; i < m; ++i)
        if (row_is_lt[i] && slack[i] > MARGIN * (1.0 + std::fabs(rhs[i]))) {
            bs.margin[n + i] = slack[i];
            cand.push_back(n + i);
        }
    if (static_cast<int64_t>(cand.size()) > m) std::nth_element(cand.begin(), cand.begin() + m, cand.end(), MarginOrder{bs.margin});
    for (size_t k = 0; k < cand.size(); ++k) {
        if (static_cast<int64_t>(k) < m) bs.is_basic[cand[k]] = 1;
        else bs.tracked.push_back(static_cast<int32_t>(cand[k]));
    }
    return cand.size();
}

// ---------------------------------------------------------------------------------------------- columns to rows
// Every band row gets at most ONE variable, whose position is the row's: a variable that sat there in the last
// factorisation and is still basic stays; a row whose own logical is basic keeps it; the other basic columns are
// matched to the free rows greedily by entry size, largest first (large entries on the diagonal, and a band no
// wider than a column is tall: a column only ever sits on a row it has an entry in).  A row no column takes holds
// a PLACEHOLDER (unit vector; border row "its value = 0"), a column that finds no row goes to the BORDER.
struct Matching {
    std::vector<int64_t> bvar;   // [band rows] the variable on the position, -1: none
    std::vector<uint8_t> placed; // [n + m] the variable has a band position
};
namespace detail {
struct Ent {
    double a;
    int32_t ib;
    int64_t var;
};
// order: size descending, then variable, then band row -- a stable LSD radix sort on the inverted bits of the
// (positive, finite or infinite) size, 16 bits a pass (8e5 candidates in ~10 ms against ~40 for std::sort with the
// three-way comparison) -- then every candidate in that order takes its row if both are still free
inline void place_sorted(std::vector<Ent> &ents, Matching &mt) {
    std::vector<Ent> tmp(ents.size());
    std::vector<uint32_t> hist(65536);
    auto key = [](const Ent &e) {
        uint64_t bits;
        std::memcpy(&bits, &e.a, sizeof(bits));
        return ~bits;
    };
    for (int pass = 0; pass < 4 && ents.size() > 1; ++pass) {
        const int sh = 16 * pass;
        std::fill(hist.begin(), hist.end(), 0u);
        for (const Ent &e : ents) ++hist[(key(e) >> sh) & 0xFFFF];
        uint32_t run = 0;
        for (uint32_t &hh_ : hist) {
            const uint32_t cc = hh_;
            hh_ = run;
            run += cc;
        }
        for (const Ent &e : ents) tmp[hist[(key(e) >> sh) & 0xFFFF]++] = e;
        ents.swap(tmp);
    }
    for (const Ent &e : ents)
        if (!mt.placed[e.var] && mt.bvar[e.ib] < 0) {
            mt.bvar[e.ib] = e.var;
            mt.placed[e.var] = 1;
        }
}
} // namespace detail
// rp: the call's rows; is_basic [n + m]; prev_pos: empty, or [band rows] from the last epoch.
inline void match_columns_to_rows(const Csc &A, const RowPlan &rp, const std::vector<uint8_t> &is_basic, const std::vector<int64_t> &prev_pos,
                                  Matching &mt) {
    using detail::Ent;
    const int64_t n = A.n, m1 = static_cast<int64_t>(rp.rows_band.size());
    std::vector<int64_t> &bvar = mt.bvar;
    std::vector<uint8_t> &placed = mt.placed;
    bvar.assign(static_cast<size_t>(m1), -1);
    placed.assign(static_cast<size_t>(n + A.m), 0);
    if (!prev_pos.empty())
        for (int64_t p = 0; p < m1; ++p) {
            const int64_t v = prev_pos[p];
            if (v >= 0 && is_basic[v] && !placed[v]) {
                bvar[p] = v;
                placed[v] = 1;
            }
        }
    for (int64_t p = 0; p < m1; ++p) {
        const int64_t v = n + rp.rows_band[p];
        if (bvar[p] < 0 && is_basic[v] && !placed[v]) {
            bvar[p] = v;
            placed[v] = 1;
        }
    }
    // Two rounds (the one sort over every entry of every column was 0.16 of the 0.41 s this set-up took at 1e6 rows:
    // 7e6 candidates of 24 bytes, four passes): first every column's LARGEST entry in a free row competes -- one
    // candidate per column, and in a column-dominant basis the winner nearly everywhere --, then the columns that lost
    // theirs compete with all their entries for the rows that are left
    std::vector<Ent> ents;
    for (int64_t j = 0; j < n; ++j) {
        if (!is_basic[j] || placed[j]) continue;
        Ent best{0.0, -1, j};
        for (int64_t k = A.ptr[j]; k < A.ptr[j + 1]; ++k) {
            const int32_t ib = rp.rowb[A.idx[k]];
            const double a = std::fabs(A.val[k]);
            if (ib >= 0 && bvar[ib] < 0 && a > MATCH_MIN && (a > best.a || (a == best.a && ib < best.ib))) best = Ent{a, ib, j};
        }
        if (best.ib >= 0) ents.push_back(best);
    }
    detail::place_sorted(ents, mt);
    ents.clear();
    for (int64_t j = 0; j < n; ++j) {
        if (!is_basic[j] || placed[j]) continue;
        const size_t first = ents.size();
        for (int64_t k = A.ptr[j]; k < A.ptr[j + 1]; ++k) {
            const int32_t ib = rp.rowb[A.idx[k]];
            const double a = std::fabs(A.val[k]);
            if (ib >= 0 && bvar[ib] < 0 && a > MATCH_MIN) ents.push_back(Ent{a, ib, j});
        }
        // a column's candidates by band row (a handful: insertion sort), so that the stable sort leaves equal sizes
        // in (variable, band row) order
        for (size_t q = first + 1; q < ents.size(); ++q) {
            const Ent e = ents[q];
            size_t r = q;
            for (; r > first && ents[r - 1].ib > e.ib; --r) ents[r] = ents[r - 1];
            ents[r] = e;
        }
    }
    detail::place_sorted(ents, mt);
}

// ---------------------------------------------------------------------------------------------- band entries, widths
// THE walk over the band part of the matched columns: for every position p that holds a column of A, f(row position,
// p, value) for its entries in band rows; kl / ku come out as the widest reach below / above the diagonal.  Positions
// that hold no column (placeholder, logical, padding) are reported as unit(p).  Used before the cut into blocks (widths
// only: they size the separators) and after it (the triplets the band LU gets).
template <class OnEntry, class OnUnit>
inline void walk_band(const Csc &A, const std::vector<int64_t> &bvar, const std::vector<int32_t> &rowb, int &kl, int &ku, OnEntry entry, OnUnit unit) {
    kl = 0;
    ku = 0;
    const int64_t m1 = static_cast<int64_t>(bvar.size());
    for (int64_t p = 0; p < m1; ++p) {
        const int64_t v = bvar[p];
        if (v < 0 || v >= A.n) {
            unit(p);
            continue;
        }
        for (int64_t k = A.ptr[v]; k < A.ptr[v + 1]; ++k) {
            const int32_t ib = rowb[A.idx[k]];
            if (ib >= 0) {
                entry(ib, p, A.val[k]);
                kl = std::max<int>(kl, ib - static_cast<int>(p));
                ku = std::max<int>(ku, static_cast<int>(p) - ib);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- blocks: the band cut at SEPARATORS
// A panel of the band LU is a chain of 32 dependent column steps on one workgroup (53 us at kl + ku = 230), a band of
// 1e5 rows 3,100 of them in a row.  Cut every RL + W positions: W = max(kl, ku) positions (rows AND the columns matched
// to them) go to the border as separators -- no column left of a separator reaches a row right of it, or the other way
// round -- so the P blocks between them are independent band matrices, factored side by side
// (sx_bandlu_factor_blocks_dev; identity padding of kl + ku + 32 positions keeps their memory apart).  The Schur
// complement grows by (P - 1) W rows.
//
// One epoch's geometry: band positions with padding, dense rows with the separators' rows.  Everything after the
// matching reads this and nothing of the RowPlan.
struct EpochGeometry {
    int64_t P = 1, RL = 0, Wsep = 0, PAD = 0, stride = 0, RL_last = 0;
    int64_t m1_all = 0;              // band rows of the call (positions before the cut)
    int64_t m1 = 0;                  // band positions of the epoch, padding included (m1e)
    int64_t ndr = 0;                 // dense rows plus separator rows
    std::vector<int64_t> bvar;       // [m1] variable on the position; -1: placeholder, -2: padding
    std::vector<int32_t> posrow;     // [m1] the row of the position (-1: padding)
    std::vector<int32_t> old_of_new; // [m1] the position before the cut (-1: padding)
    std::vector<int32_t> rows_dense; // [ndr]
    std::vector<int32_t> rowb;       // [m] row -> band position, -1: border row
    std::vector<int32_t> eqidx;      // [m] row -> position in [band positions, border rows]
};
inline int64_t default_block_count(int64_t m1_all) { return std::min<int64_t>(32, m1_all / 8192); }
// mt: the matching over rp (its `placed` loses the separators' columns).  want: requested block count; as many as the
// widths allow are taken (2,048 rows of the border are left to placeholders and columns without a row).
inline void make_geometry(const Csc &A, const RowPlan &rp, Matching &mt, int64_t want, EpochGeometry &g) {
    const int64_t m1_all = static_cast<int64_t>(rp.rows_band.size()), ndr0 = static_cast<int64_t>(rp.rows_dense.size());
    int kl0 = 0, ku0 = 0;
    walk_band(A, mt.bvar, rp.rowb, kl0, ku0, [](int32_t, int64_t, double) {}, [](int64_t) {});
    const int64_t w = std::max(kl0, ku0), pad = ((kl0 + ku0 + 32 + 31) / 32) * 32;
    g = EpochGeometry{};
    g.m1_all = m1_all;
    g.RL = m1_all;
    while (want > 1) {
        const int64_t rl = ((m1_all - (want - 1) * w) / want) / 32 * 32;
        if (w > 0 && rl >= 4 * pad && ndr0 + (want - 1) * w + 2048 <= MAX_NB) break;
        --want;
    }
    if (want > 1) {
        g.P = want;
        g.Wsep = w;
        g.PAD = pad;
        g.RL = ((m1_all - (g.P - 1) * w) / g.P) / 32 * 32;
    }
    const int64_t P = g.P, RL = g.RL, Wsep = g.Wsep;
    g.RL_last = m1_all - (P - 1) * (RL + Wsep);
    g.stride = RL + g.PAD;
    g.m1 = (P - 1) * g.stride + g.RL_last;
    const int64_t nsep = (P - 1) * Wsep;
    g.ndr = ndr0 + nsep;
    g.bvar.assign(static_cast<size_t>(g.m1), -2); // (-2: padding, -1: placeholder)
    g.posrow.assign(static_cast<size_t>(g.m1), -1);
    g.old_of_new.assign(static_cast<size_t>(g.m1), -1);
    g.rows_dense = rp.rows_dense;
    g.rows_dense.resize(static_cast<size_t>(g.ndr));
    g.rowb.assign(static_cast<size_t>(A.m), -1);
    g.eqidx.assign(static_cast<size_t>(A.m), 0);
    for (int64_t p = 0; p < m1_all; ++p) {
        const int64_t blk = std::min<int64_t>(p / (RL + Wsep), P - 1), off = p - blk * (RL + Wsep);
        const int32_t row = rp.rows_band[p];
        if (blk < P - 1 && off >= RL) { // a separator: its row joins the dense rows, its column goes to the border
            g.rows_dense[static_cast<size_t>(ndr0 + blk * Wsep + off - RL)] = row;
            if (mt.bvar[p] >= 0) mt.placed[mt.bvar[p]] = 0;
            continue;
        }
        const int64_t np = blk * g.stride + off;
        g.bvar[np] = mt.bvar[p];
        g.posrow[np] = row;
        g.old_of_new[np] = static_cast<int32_t>(p);
        g.rowb[row] = static_cast<int32_t>(np);
        g.eqidx[row] = static_cast<int32_t>(np);
    }
    for (size_t k = 0; k < g.rows_dense.size(); ++k) g.eqidx[g.rows_dense[k]] = static_cast<int32_t>(g.m1 + static_cast<int64_t>(k));
}

// band triplets (a placeholder, a logical or padding: the unit vector of the position), band widths
struct BandTriplets {
    std::vector<int32_t> row, col;
    std::vector<double> val;
    int kl = 0, ku = 0;
};
inline void band_triplets(const Csc &A, int64_t nnz, const EpochGeometry &g, BandTriplets &t) {
    t.row.clear();
    t.col.clear();
    t.val.clear();
    t.row.reserve(static_cast<size_t>(nnz) / 2 + static_cast<size_t>(g.m1));
    t.col.reserve(t.row.capacity());
    t.val.reserve(t.row.capacity());
    auto push = [&t](int32_t r, int64_t p, double v) {
        t.row.push_back(r);
        t.col.push_back(static_cast<int32_t>(p));
        t.val.push_back(v);
    };
    walk_band(A, g.bvar, g.rowb, t.kl, t.ku, push, [&push](int64_t p) { push(static_cast<int32_t>(p), p, 1.0); });
}

// ---------------------------------------------------------------------------------------------- after the band LU
// rep [m1]: the LU replaced column j by a unit vector; piv [m1]: the row swapped onto the diagonal at step j.
// A replaced column stands for the unit vector of the row that sat on its diagonal: a placeholder; the column
// itself goes to the border.  ph_row [m1]: the row whose unit vector a placeholder is (-1: no placeholder).
inline void after_band_lu(EpochGeometry &g, Matching &mt, const std::vector<int32_t> &rep, const std::vector<int32_t> &piv, std::vector<int32_t> &ph_row) {
    std::vector<int32_t> rowof(static_cast<size_t>(g.m1));
    std::iota(rowof.begin(), rowof.end(), 0);
    for (int64_t j = 0; j < g.m1; ++j) {
        if (rep[j]) {
            if (g.bvar[j] >= 0) mt.placed[g.bvar[j]] = 0;
            g.bvar[j] = -1;
            ph_row[j] = g.posrow[rowof[j]];
        } else {
            if (piv[j] != j) std::swap(rowof[j], rowof[piv[j]]);
            if (g.bvar[j] == -1) ph_row[j] = g.posrow[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------- the border: as many columns as rows
struct Border {
    std::vector<int64_t> bcol;   // [nb] the border's columns (-1 after the dense LU: the mirror image of a placeholder that became a logical)
    int64_t h = 0;               // placeholders
    std::vector<int32_t> ph_pos; // [h] their positions
    int64_t nb(const EpochGeometry &g) const { return g.ndr + h; }
};
// Too few columns for the border rows (or a border beyond the dense LU): placeholders become their row's own
// logical, then the dense rows' logicals fill in; too many: the surplus leaves the basis (superbasic).  With by_margin
// (a guessed basis) the border takes its columns in the order of their margins.  Returns false when the border still does
// not have ndr + h columns or exceeds MAX_NB rows (the caller reports g.ndr + bd.h, bd.bcol.size(), MAX_NB).
inline bool balance_border(int64_t n, EpochGeometry &g, Matching &mt, const std::vector<int32_t> &ph_row, bool by_margin, BasisState &bs, Border &bd) {
    const int64_t NV = static_cast<int64_t>(bs.is_basic.size()), m1 = g.m1, ndr = g.ndr;
    std::vector<int64_t> &bcol = bd.bcol;
    bcol.clear();
    for (int64_t v = 0; v < NV; ++v)
        if (bs.is_basic[v] && !mt.placed[v]) bcol.push_back(v);
    int64_t h = 0;
    for (int64_t p = 0; p < m1; ++p) h += g.bvar[p] == -1;
    std::vector<int32_t> gone;
    for (int64_t p = 0; p < m1 && (static_cast<int64_t>(bcol.size()) < ndr + h || ndr + h > MAX_NB); ++p) {
        if (g.bvar[p] != -1) continue;
        const int64_t w = n + ph_row[p];
        if (bs.is_basic[w]) continue;
        g.bvar[p] = w;
        bs.is_basic[w] = 1;
        mt.placed[w] = 1;
        gone.push_back(static_cast<int32_t>(w));
        --h;
    }
    for (int64_t k = 0; k < ndr && static_cast<int64_t>(bcol.size()) < ndr + h; ++k) {
        const int64_t w = n + g.rows_dense[k];
        if (bs.is_basic[w]) continue;
        bs.is_basic[w] = 1;
        bcol.push_back(w);
        gone.push_back(static_cast<int32_t>(w));
    }
    if (!gone.empty()) {
        std::vector<uint8_t> gflag(static_cast<size_t>(NV), 0);
        for (int32_t w : gone) gflag[w] = 1;
        bs.tracked.erase(std::remove_if(bs.tracked.begin(), bs.tracked.end(), [&](int32_t v) { return gflag[v] != 0; }), bs.tracked.end());
    }
    if (by_margin && !bs.margin.empty()) // the surest columns first: a column the dense LU sets aside is one of the doubtful ones
        std::sort(bcol.begin(), bcol.end(), MarginOrder{bs.margin});
    else std::sort(bcol.begin(), bcol.end());
    while (static_cast<int64_t>(bcol.size()) > ndr + h) {
        const int64_t v = bcol.back();
        bcol.pop_back();
        bs.is_basic[v] = 0;
        bs.tracked.push_back(static_cast<int32_t>(v));
    }
    bd.h = h;
    bd.ph_pos.clear();
    if (static_cast<int64_t>(bcol.size()) != ndr + h || ndr + h > MAX_NB) return false;
    for (int64_t p = 0; p < m1; ++p)
        if (g.bvar[p] == -1) bd.ph_pos.push_back(static_cast<int32_t>(p));
    return true;
}

// ---------------------------------------------------------------------------------------------- after the dense LU
// rep2 [nb]: the LU of the Schur complement found no pivot for border column j; perm2 [nb]: the border row on its diagonal.
// A border column without a pivot leaves the basis (it stays in the tableau); what takes its place is the unit
// vector of the border row on its diagonal: a dense row's logical -- or, for a placeholder's row, the
// placeholder turns into its row's real logical (and the border column into its mirror image, a dummy)
// (all of them leave first: the logical a replaced column stands for may itself be a later border column that
//  the same elimination set aside).  Returns -1, or the row whose logical the repair wanted twice.
inline int64_t after_dense_lu(int64_t n, EpochGeometry &g, const std::vector<int32_t> &ph_row, const std::vector<int32_t> &rep2,
                              const std::vector<int32_t> &perm2, BasisState &bs, Border &bd) {
    const int64_t nb = static_cast<int64_t>(bd.bcol.size());
    for (int64_t j = 0; j < nb; ++j)
        if (rep2[j]) {
            bs.is_basic[bd.bcol[j]] = 0;
            bs.tracked.push_back(static_cast<int32_t>(bd.bcol[j]));
        }
    for (int64_t j = 0; j < nb; ++j) {
        if (!rep2[j]) continue;
        const int64_t r = perm2[j];
        int64_t w;
        if (r < g.ndr) {
            w = n + g.rows_dense[r];
            bd.bcol[j] = w;
        } else {
            const int64_t p = bd.ph_pos[static_cast<size_t>(r - g.ndr)];
            w = n + ph_row[p];
            g.bvar[p] = w;
            bd.bcol[j] = -1;
        }
        if (bs.is_basic[w]) return w - n;
        bs.is_basic[w] = 1;
        bs.tracked.erase(std::remove(bs.tracked.begin(), bs.tracked.end(), static_cast<int32_t>(w)), bs.tracked.end());
    }
    return -1;
}

// ---------------------------------------------------------------------------------------------- B21, B12
// B21: the dense rows' entries in the band columns, one unit entry per placeholder row -- by border row (rows) and by band
// position (cols, compact)
inline void b21_blocks(const Csc &A, const EpochGeometry &g, const Border &bd, HostRows &rows, HostRows &cols) {
    std::vector<int32_t> er, ep;
    std::vector<double> ev;
    for (int64_t p = 0; p < g.m1; ++p) {
        const int64_t v = g.bvar[p];
        if (v < 0 || v >= A.n) continue;
        for (int64_t k = A.ptr[v]; k < A.ptr[v + 1]; ++k)
            if (g.rowb[A.idx[k]] < 0) {
                er.push_back(g.eqidx[A.idx[k]] - static_cast<int32_t>(g.m1));
                ep.push_back(static_cast<int32_t>(p));
                ev.push_back(A.val[k]);
            }
    }
    for (size_t t = 0; t < bd.ph_pos.size(); ++t) {
        er.push_back(static_cast<int32_t>(g.ndr + static_cast<int64_t>(t)));
        ep.push_back(bd.ph_pos[t]);
        ev.push_back(1.0);
    }
    rows_from_triplets(bd.nb(g), er, ep, ev, false, rows);
    rows_from_triplets(g.m1, ep, er, ev, true, cols);
}
// B12: the border columns' entries in the band rows -- by band position (rows, compact) and by border column (cols)
inline void b12_blocks(const Csc &A, const EpochGeometry &g, const Border &bd, HostRows &rows, HostRows &cols) {
    const int64_t nb = bd.nb(g);
    std::vector<int32_t> ep, ej;
    std::vector<double> ev;
    for (int64_t j = 0; j < nb; ++j) {
        const int64_t v = bd.bcol[j];
        if (v < 0) continue;
        if (v >= A.n) {
            if (g.rowb[v - A.n] >= 0) {
                ep.push_back(g.rowb[v - A.n]);
                ej.push_back(static_cast<int32_t>(j));
                ev.push_back(1.0);
            }
            continue;
        }
        for (int64_t k = A.ptr[v]; k < A.ptr[v + 1]; ++k)
            if (g.rowb[A.idx[k]] >= 0) {
                ep.push_back(g.rowb[A.idx[k]]);
                ej.push_back(static_cast<int32_t>(j));
                ev.push_back(A.val[k]);
            }
    }
    rows_from_triplets(g.m1, ep, ej, ev, true, rows);
    rows_from_triplets(nb, ej, ep, ev, false, cols);
}

// ---------------------------------------------------------------------------------------------- who is where
// head [m1 + nb]: the variable on each position of the factored basis (< 0: a dummy -- placeholder, padding or mirror
// column); bs.vstat / bs.is_basic follow it; varJ: the tracked columns that are not basic, in the order of the variables.
// Returns 0, 1 (variable `bad` covers two positions) or 2 (`bad` basic variables instead of m).
inline int who_is_where(int64_t m, const EpochGeometry &g, const Border &bd, BasisState &bs, std::vector<int64_t> &head, std::vector<int32_t> &varJ,
                        int64_t &n_dummy, int64_t &bad) {
    const int64_t nb = bd.nb(g), mp = g.m1 + nb, NV = static_cast<int64_t>(bs.vstat.size());
    head.assign(static_cast<size_t>(mp), -1);
    for (int64_t p = 0; p < g.m1; ++p) head[p] = g.bvar[p];
    for (int64_t j = 0; j < nb; ++j) head[g.m1 + j] = bd.bcol[j];
    std::fill(bs.vstat.begin(), bs.vstat.end(), 0);
    int64_t n_basic = 0;
    n_dummy = 0;
    for (int64_t p = 0; p < mp; ++p) {
        if (head[p] < 0) {
            ++n_dummy;
            continue;
        }
        if (bs.vstat[head[p]] == 1) {
            bad = head[p];
            return 1;
        }
        bs.vstat[head[p]] = 1;
        ++n_basic;
    }
    if (n_basic != m) {
        bad = n_basic;
        return 2;
    }
    for (int64_t v = 0; v < NV; ++v) bs.is_basic[v] = bs.vstat[v] == 1;
    varJ.clear();
    for (int32_t v : bs.tracked)
        if (bs.vstat[v] == 0) {
            bs.vstat[v] = 2;
            varJ.push_back(v);
        }
    std::sort(varJ.begin(), varJ.end()); // (neighbours in the order of the variables share the panels of a sparse band solve)
    return 0;
}

} // namespace sx_plan
