// Device side of two stages of the sparse crossover's set-up (K16s; the host statement is sx_band_plan.h):
//
//   sx_band_match_dev      = sx_plan::match_columns_to_rows -- every band row gets at most one basic variable;
//   sx_band_triplets_dev   = sx_plan::walk_band + sx_plan::band_triplets -- the (row, column, value) triplets of the matched
//                            band and its widths kl / ku, as sx_bandlu_create_dev takes them.
//
// MATCHING.  The host sorts candidates by (size descending, variable, band row) and lets each one take its row if both ends are
// still free -- twice: first one candidate per column, then every entry of the columns that lost.  A greedy pass over a total
// order places exactly the edges that are LOCALLY DOMINANT (first of both their column and their row among what remains), so
// the same matching comes out of parallel rounds, whatever the schedule:
//   seeds    a position keeps prev_pos[p] while that variable is basic (launch 1); then a free position whose own row's logical
//            is basic and unplaced takes it (launch 2 -- it has to see what launch 1 placed: prev_pos may hold a logical on
//            another position than its row's).  prev_pos names a variable at most once: the driver's invariant
//            (sx_plan::who_is_where refuses a variable on two positions), relied on here -- the host's `!placed[v]` test in its
//            first loop only matters without it;
//   round 1  every basic, unplaced column proposes its largest entry in a free row (ties: smaller row); every row takes its
//            best proposer (ties: smaller variable).  Each column proposes once: one pass;
//   round 2  over the columns that proposed and lost, COMPACTED ONCE into a list: each finds its best remaining edge, each free
//            row the best remaining edge into it, and an edge that is both is placed; again until a round finds no edge.
//            The count depends on the data (a chain of columns that each wait for their neighbour takes one round per column),
//            so rounds are launched in groups of BM_GROUP -- the first group directly, further ones as ONE captured graph
//            replayed (sx_graph.h) -- with a device flag that makes the rounds after the last one return at once; the host
//            reads the flag between groups.
// Work split: BM_G = 8 lanes per column (a column of a sub-problem has a handful of entries: a wave per column idles 60
// lanes, a lane per column walks eight cache lines of its own); lane s takes entries s, s + 8, ..., the eight partial bests
// meet by __shfl_xor inside the group.  No kernel has a barrier, so a dense column costs its own lane group len / 8 steps and
// holds nobody else up.
// Row winner: per band row a 64-bit key reduced by VECTOR atomics -- atomicMax on the bit pattern of |a| (positive doubles
// order like their bits), then, in a second launch, atomicMin on the variable among the edges whose size equals that maximum.
// Both are order-free reductions: the result does not depend on scheduling.  Two key sets alternate between rounds; a round
// clears the other set on exactly the rows its columns can still reach (a superset of what the next round touches: columns
// and free rows only ever leave), so no pass over all rows is needed between rounds.
//
// ASSEMBLY.  Count (lane group per position) -> exclusive scan -> fill at the scanned offsets, the entries of a column in
// their stored order (ballot compaction inside the lane group): the triplets come out in the order of the host walk.  That
// order is not needed: k_gb_scatter (sx_bandlu.hip) writes AB(i, j) = val[t] with one work-item per triplet and no
// accumulation, every (row, column) pair occurs once (one column per position, one entry per row in a column), so the band
// matrix is the same for any order of the triplets.  kl / ku: wave maximum, then atomicMax.
#include "sx_internal.h"
#include "sx_graph.h"
#include "sx_band_plan.h"

#include <algorithm>

namespace {

constexpr int BM_WG = 256;
constexpr int BM_G = 8;     // lanes per column
constexpr int BM_GROUP = 8; // mutual-best rounds per launch group (even: the two key sets alternate)
constexpr unsigned long long BM_NOVAR = ~0ull;
constexpr int BM_NOROW = 0x7fffffff;

struct BmState {
    int done;         // a mutual-best round found no edge: later rounds return at once
    int any;          // this round saw an edge
    int n_list;       // columns that proposed in round 1 and lost
    int pad;
    long long rounds; // mutual-best rounds that placed something
};

inline unsigned bm_grid(int64_t threads) { return static_cast<unsigned>(threads > 0 ? (threads + BM_WG - 1) / BM_WG : 1); }

// the better of two candidates of ONE column: larger size, then smaller band row (none: size 0, row BM_NOROW)
__device__ __forceinline__ void bm_take(unsigned long long &a, int &ib, unsigned long long oa, int oib) {
    if (oa > a || (oa == a && oib < ib)) {
        a = oa;
        ib = oib;
    }
}
__device__ __forceinline__ void bm_group_best(unsigned long long &a, int &ib) {
#pragma unroll
    for (int o = BM_G / 2; o > 0; o >>= 1) {
        const unsigned long long oa = __shfl_xor(a, o, BM_G);
        const int oib = __shfl_xor(ib, o, BM_G);
        bm_take(a, ib, oa, oib);
    }
}

struct BmCsc {
    int64_t m, n;
    const int64_t *ptr;
    const int32_t *idx;
    const double *val;
};

// lane `sub` of column j's group over its share of the column: best entry in a free band row; ROW_KEYS: every such entry also
// bids for its row (round 2: a row looks at all remaining edges, round 1 only at the one each column proposes)
template <bool ROW_KEYS>
__device__ __forceinline__ void bm_scan(const BmCsc &A, int64_t j, int sub, const int32_t *__restrict__ rowb, int64_t m1,
                                        const int64_t *__restrict__ bvar, unsigned long long *__restrict__ rowkey, unsigned long long &a,
                                        int &ib) {
    a = 0ull;
    ib = BM_NOROW;
    for (int64_t k = A.ptr[j] + sub; k < A.ptr[j + 1]; k += BM_G) {
        const int r = rowb[A.idx[k]];
        const double x = fabs(A.val[k]);
        if (r < 0 || r >= m1 || !(x > sx_plan::MATCH_MIN) || bvar[r] >= 0) continue;
        const unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(x));
        if (ROW_KEYS) atomicMax(&rowkey[r], bits);
        bm_take(a, ib, bits, r);
    }
}

// ---------------------------------------------------------------------------------------------- start, seeds
__global__ __launch_bounds__(BM_WG) void k_bm_init(int64_t m1, int64_t nv, int64_t *__restrict__ bvar, uint8_t *__restrict__ placed,
                                                   unsigned long long *__restrict__ rowkey, unsigned long long *__restrict__ rowvar,
                                                   BmState *__restrict__ st) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * BM_WG + threadIdx.x;
    if (t < m1) bvar[t] = -1;
    if (t < nv) placed[t] = 0;
    if (t < 2 * m1) {
        rowkey[t] = 0ull;
        rowvar[t] = BM_NOVAR;
    }
    if (t == 0) *st = BmState{0, 0, 0, 0, 0};
}

__global__ __launch_bounds__(BM_WG) void k_bm_seed_prev(int64_t m1, int64_t nv, const int64_t *__restrict__ prev_pos,
                                                        const uint8_t *__restrict__ is_basic, int64_t *__restrict__ bvar,
                                                        uint8_t *__restrict__ placed) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * BM_WG + threadIdx.x;
    if (p >= m1) return;
    const int64_t v = prev_pos[p];
    if (v >= 0 && v < nv && is_basic[v]) {
        bvar[p] = v;
        placed[v] = 1;
    }
}

// one lane per ROW (rowb is one-to-one on the band rows: a lane owns its position and its logical)
__global__ __launch_bounds__(BM_WG) void k_bm_seed_logical(int64_t m, int64_t n, int64_t m1, const int32_t *__restrict__ rowb,
                                                           const uint8_t *__restrict__ is_basic, int64_t *__restrict__ bvar,
                                                           uint8_t *__restrict__ placed) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * BM_WG + threadIdx.x;
    if (i >= m) return;
    const int p = rowb[i];
    if (p < 0 || p >= m1) return;
    if (bvar[p] < 0 && is_basic[n + i] && !placed[n + i]) {
        bvar[p] = n + i;
        placed[n + i] = 1;
    }
}

// ---------------------------------------------------------------------------------------------- round 1
__global__ __launch_bounds__(BM_WG) void k_bm_r1_best(BmCsc A, const uint8_t *__restrict__ is_basic, const uint8_t *__restrict__ placed,
                                                      const int32_t *__restrict__ rowb, int64_t m1, const int64_t *__restrict__ bvar,
                                                      unsigned long long *__restrict__ rowkey, unsigned long long *__restrict__ cbits,
                                                      int32_t *__restrict__ cib) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * BM_WG + threadIdx.x;
    const int64_t j = t / BM_G;
    const int sub = static_cast<int>(t % BM_G);
    unsigned long long a = 0ull;
    int ib = BM_NOROW;
    if (j < A.n && is_basic[j] && !placed[j]) bm_scan<false>(A, j, sub, rowb, m1, bvar, rowkey, a, ib);
    bm_group_best(a, ib);
    if (sub != 0 || j >= A.n) return;
    cbits[j] = a;
    cib[j] = a ? ib : -1;
    if (a) atomicMax(&rowkey[ib], a);
}

// among the proposers of a row whose size is the row's maximum: the smallest variable
__global__ __launch_bounds__(BM_WG) void k_bm_r1_var(int64_t n, const unsigned long long *__restrict__ cbits, const int32_t *__restrict__ cib,
                                                     const unsigned long long *__restrict__ rowkey, unsigned long long *__restrict__ rowvar) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * BM_WG + threadIdx.x;
    if (j >= n) return;
    const int ib = cib[j];
    if (ib >= 0 && cbits[j] == rowkey[ib]) atomicMin(&rowvar[ib], static_cast<unsigned long long>(j));
}

// the row's choice takes it; a proposer that lost joins the list of round 2 (one atomicAdd per wave; the order of the list
// decides nothing).  A column that had nothing to propose has no entry in a free row now and will have none later.
__global__ __launch_bounds__(BM_WG) void k_bm_r1_place(int64_t n, const unsigned long long *__restrict__ cbits, const int32_t *__restrict__ cib,
                                                       const unsigned long long *__restrict__ rowkey, const unsigned long long *__restrict__ rowvar,
                                                       int64_t *__restrict__ bvar, uint8_t *__restrict__ placed, int32_t *__restrict__ list,
                                                       BmState *__restrict__ st) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * BM_WG + threadIdx.x;
    bool lost = false;
    if (j < n) {
        const int ib = cib[j];
        if (ib >= 0) {
            if (cbits[j] == rowkey[ib] && rowvar[ib] == static_cast<unsigned long long>(j)) {
                bvar[ib] = j;
                placed[j] = 1;
            } else lost = true;
        }
    }
    const unsigned long long bal = __ballot(lost);
    if (bal == 0ull) return;
    const int lane = threadIdx.x & 63, first = __ffsll(static_cast<long long>(bal)) - 1;
    int base = 0;
    if (lane == first) base = atomicAdd(&st->n_list, __popcll(bal));
    base = __shfl(base, first, 64);
    if (lost) list[base + __popcll(bal & ((1ull << lane) - 1ull))] = static_cast<int32_t>(j);
}

// ---------------------------------------------------------------------------------------------- round 2: one mutual-best round
// key / var: this round's set; okey / ovar: the other one, cleared here for the next round
__global__ __launch_bounds__(BM_WG) void k_bm_col_best(BmCsc A, int nl, const int32_t *__restrict__ list, const uint8_t *__restrict__ placed,
                                                       const int32_t *__restrict__ rowb, int64_t m1, const int64_t *__restrict__ bvar,
                                                       unsigned long long *__restrict__ key, unsigned long long *__restrict__ cbits,
                                                       int32_t *__restrict__ cib, BmState *__restrict__ st) {
    if (st->done) return;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * BM_WG + threadIdx.x;
    const int64_t e = t / BM_G;
    const int sub = static_cast<int>(t % BM_G);
    unsigned long long a = 0ull;
    int ib = BM_NOROW;
    if (e < nl) {
        const int64_t j = list[e];
        if (!placed[j]) bm_scan<true>(A, j, sub, rowb, m1, bvar, key, a, ib);
    }
    bm_group_best(a, ib);
    if (sub != 0 || e >= nl) return;
    cbits[e] = a;
    cib[e] = a ? ib : -1;
    if (a) st->any = 1; // (every writer stores 1)
}

__global__ __launch_bounds__(BM_WG) void k_bm_row_var(BmCsc A, int nl, const int32_t *__restrict__ list, const uint8_t *__restrict__ placed,
                                                      const int32_t *__restrict__ rowb, int64_t m1, const int64_t *__restrict__ bvar,
                                                      const unsigned long long *__restrict__ key, unsigned long long *__restrict__ var,
                                                      unsigned long long *__restrict__ okey, unsigned long long *__restrict__ ovar,
                                                      const BmState *__restrict__ st) {
    if (st->done) return;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * BM_WG + threadIdx.x;
    const int64_t e = t / BM_G;
    if (e >= nl) return;
    const int64_t j = list[e];
    if (placed[j]) return;
    for (int64_t k = A.ptr[j] + t % BM_G; k < A.ptr[j + 1]; k += BM_G) {
        const int r = rowb[A.idx[k]];
        const double x = fabs(A.val[k]);
        if (r < 0 || r >= m1 || !(x > sx_plan::MATCH_MIN) || bvar[r] >= 0) continue;
        if (static_cast<unsigned long long>(__double_as_longlong(x)) == key[r]) atomicMin(&var[r], static_cast<unsigned long long>(j));
        okey[r] = 0ull; // (every writer stores the same)
        ovar[r] = BM_NOVAR;
    }
}

__global__ __launch_bounds__(BM_WG) void k_bm_place(int nl, const int32_t *__restrict__ list, const unsigned long long *__restrict__ cbits,
                                                    const int32_t *__restrict__ cib, const unsigned long long *__restrict__ key,
                                                    const unsigned long long *__restrict__ var, int64_t *__restrict__ bvar,
                                                    uint8_t *__restrict__ placed, BmState *__restrict__ st) {
    if (st->done) return; // (set below only by a round without an edge: a workgroup that sees it early has nothing to place)
    const int64_t e = static_cast<int64_t>(blockIdx.x) * BM_WG + threadIdx.x;
    if (e < nl) {
        const int ib = cib[e];
        const int64_t j = list[e];
        if (ib >= 0 && cbits[e] == key[ib] && var[ib] == static_cast<unsigned long long>(j)) {
            bvar[ib] = j;
            placed[j] = 1;
        }
    }
    if (e == 0) { // the round's verdict (`any` was written by k_bm_col_best alone)
        const int any = st->any;
        st->rounds += any;
        st->any = 0;
        st->done = any ? 0 : 1;
    }
}

// ---------------------------------------------------------------------------------------------- band assembly
__global__ __launch_bounds__(BM_WG) void k_bt_count(int64_t m1, BmCsc A, const int64_t *__restrict__ bvar, const int32_t *__restrict__ rowb,
                                                    int64_t *__restrict__ cnt, int *__restrict__ wid) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * BM_WG + threadIdx.x;
    const int64_t p = t / BM_G;
    const int sub = static_cast<int>(t % BM_G);
    int c = 0, kl = 0, ku = 0;
    if (p < m1) {
        const int64_t v = bvar[p];
        if (v < 0 || v >= A.n) c = sub == 0 ? 1 : 0; // placeholder, padding, logical: the unit vector of the position
        else
            for (int64_t k = A.ptr[v] + sub; k < A.ptr[v + 1]; k += BM_G) {
                const int r = rowb[A.idx[k]];
                if (r < 0) continue;
                ++c;
                const int d = r - static_cast<int>(p);
                kl = d > kl ? d : kl;
                ku = -d > ku ? -d : ku;
            }
    }
#pragma unroll
    for (int o = BM_G / 2; o > 0; o >>= 1) c += __shfl_xor(c, o, BM_G);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int okl = __shfl_xor(kl, o, 64), oku = __shfl_xor(ku, o, 64);
        kl = okl > kl ? okl : kl;
        ku = oku > ku ? oku : ku;
    }
    if (sub == 0 && p < m1) cnt[p] = c;
    if ((threadIdx.x & 63) == 0) {
        if (kl > 0) atomicMax(&wid[0], kl);
        if (ku > 0) atomicMax(&wid[1], ku);
    }
}

__global__ __launch_bounds__(BM_WG) void k_bt_fill(int64_t m1, BmCsc A, const int64_t *__restrict__ bvar, const int32_t *__restrict__ rowb,
                                                   const int64_t *__restrict__ offs, int32_t *__restrict__ trow, int32_t *__restrict__ tcol,
                                                   double *__restrict__ tval) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * BM_WG + threadIdx.x;
    const int64_t p = t / BM_G;
    const int sub = static_cast<int>(t % BM_G);
    if (p >= m1) return;
    const int64_t v = bvar[p];
    int64_t o = offs[p];
    if (v < 0 || v >= A.n) {
        if (sub == 0) {
            trow[o] = static_cast<int32_t>(p);
            tcol[o] = static_cast<int32_t>(p);
            tval[o] = 1.0;
        }
        return;
    }
    const int shift = (threadIdx.x & 63) & ~(BM_G - 1); // the group's lanes inside the wave's ballot
    const int64_t k1 = A.ptr[v + 1];
    for (int64_t k0 = A.ptr[v]; k0 < k1; k0 += BM_G) { // (uniform inside the group)
        const int64_t k = k0 + sub;
        const int r = k < k1 ? rowb[A.idx[k]] : -1;
        const unsigned mine = static_cast<unsigned>(__ballot(r >= 0) >> shift) & ((1u << BM_G) - 1u);
        if (r >= 0) {
            const int64_t q = o + __popc(mine & ((1u << sub) - 1u));
            trow[q] = r;
            tcol[q] = static_cast<int32_t>(p);
            tval[q] = A.val[k];
        }
        o += __popc(mine);
    }
}

inline BmCsc bm_csc(const sx_matrix *A) { return BmCsc{A->m, A->n, A->csc_ptr, A->csc_idx, A->csc_val}; }

} // namespace

// sx_plan::match_columns_to_rows on the device (include/sxhip.h)
SX_API int sx_band_match_dev(sx_ctx *ctx, const sx_matrix *A, const uint8_t *is_basic, const int32_t *rowb, int64_t m1,
                             const int64_t *prev_pos, int64_t *bvar, uint8_t *placed, int64_t *rounds_host) {
    SX_ENTER(ctx);
    SX_REQUIRE(A && is_basic && rowb && placed && (bvar || m1 == 0), "NULL argument");
    SX_REQUIRE(A->csc_ptr != nullptr, "the matching reads the columns of A");
    SX_REQUIRE(m1 >= 0 && m1 <= A->m && A->m + A->n < 2000000000LL, "problem size");
    const int64_t m = A->m, n = A->n, nv = n + m;
    hipStream_t s = ctx->stream;
    const BmCsc csc = bm_csc(A);
    sx_stage tmp(ctx);
    unsigned long long *rowkey = nullptr, *rowvar = nullptr, *cbits = nullptr;
    int32_t *cib = nullptr, *list = nullptr;
    BmState *st = nullptr;
    SX_TRY(tmp.tmp(2 * static_cast<size_t>(m1), &rowkey));
    SX_TRY(tmp.tmp(2 * static_cast<size_t>(m1), &rowvar));
    SX_TRY(tmp.tmp(static_cast<size_t>(n), &cbits));
    SX_TRY(tmp.tmp(static_cast<size_t>(n), &cib));
    SX_TRY(tmp.tmp(static_cast<size_t>(n), &list));
    SX_TRY(tmp.tmp(1, &st));
    unsigned long long *key[2] = {rowkey, rowkey + m1}, *var[2] = {rowvar, rowvar + m1};
    hipLaunchKernelGGL(k_bm_init, dim3(bm_grid(std::max(nv, 2 * m1))), dim3(BM_WG), 0, s, m1, nv, bvar, placed, rowkey, rowvar, st);
    if (prev_pos) hipLaunchKernelGGL(k_bm_seed_prev, dim3(bm_grid(m1)), dim3(BM_WG), 0, s, m1, nv, prev_pos, is_basic, bvar, placed);
    hipLaunchKernelGGL(k_bm_seed_logical, dim3(bm_grid(m)), dim3(BM_WG), 0, s, m, n, m1, rowb, is_basic, bvar, placed);
    // round 1 on key set 0
    hipLaunchKernelGGL(k_bm_r1_best, dim3(bm_grid(n * BM_G)), dim3(BM_WG), 0, s, csc, is_basic, placed, rowb, m1, bvar, key[0], cbits, cib);
    hipLaunchKernelGGL(k_bm_r1_var, dim3(bm_grid(n)), dim3(BM_WG), 0, s, n, cbits, cib, key[0], var[0]);
    hipLaunchKernelGGL(k_bm_r1_place, dim3(bm_grid(n)), dim3(BM_WG), 0, s, n, cbits, cib, key[0], var[0], bvar, placed, list, st);
    BmState h{};
    SX_HIP(hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, s));
    SX_HIP(hipStreamSynchronize(s));
    SX_HIP(hipGetLastError());
    const int nl = h.n_list;
    // round 2: set 1 first (untouched since k_bm_init), the sets alternate from round to round
    auto group = [&]() {
        for (int r = 0; r < BM_GROUP; ++r) {
            const int cur = (r + 1) & 1, oth = r & 1;
            hipLaunchKernelGGL(k_bm_col_best, dim3(bm_grid(static_cast<int64_t>(nl) * BM_G)), dim3(BM_WG), 0, s, csc, nl, list, placed, rowb, m1, bvar,
                               key[cur], cbits, cib, st);
            hipLaunchKernelGGL(k_bm_row_var, dim3(bm_grid(static_cast<int64_t>(nl) * BM_G)), dim3(BM_WG), 0, s, csc, nl, list, placed, rowb, m1, bvar,
                               key[cur], var[cur], key[oth], var[oth], st);
            hipLaunchKernelGGL(k_bm_place, dim3(bm_grid(nl)), dim3(BM_WG), 0, s, nl, list, cbits, cib, key[cur], var[cur], bvar, placed, st);
        }
    };
    SxGraphBatch batch;
    bool try_graph = sx_graph_wanted(ctx, SX_GRAPH_HEED_NO_GRAPH_ENV | SX_GRAPH_HEED_PROFILER);
    // every round with an edge places one, so there are at most m1 of them and one more that finds none
    for (int64_t g = 0; nl > 0 && !h.done; ++g) {
        SX_REQUIRE(g * BM_GROUP <= m1, "internal: the matching rounds do not end");
        if (g > 0 && try_graph && !batch.ready()) try_graph = batch.capture(s, group); // (the first group covers the usual two or three rounds)
        if (g > 0 && batch.ready()) SX_HIP(batch.launch(s));
        else group();
        SX_HIP(hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, s));
        SX_HIP(hipStreamSynchronize(s));
        SX_HIP(hipGetLastError());
    }
    if (rounds_host) *rounds_host = h.rounds;
    return SX_OK;
}

// sx_plan::walk_band + sx_plan::band_triplets on the device (include/sxhip.h)
SX_API int sx_band_triplets_dev(sx_ctx *ctx, const sx_matrix *A, int64_t m1, const int64_t *bvar, const int32_t *rowb, int64_t cap,
                                int32_t *row, int32_t *col, double *val, int64_t *count_host, int *kl_host, int *ku_host) {
    SX_ENTER(ctx);
    SX_REQUIRE(A && bvar && rowb, "NULL argument");
    SX_REQUIRE(A->csc_ptr != nullptr, "the band assembly reads the columns of A");
    SX_REQUIRE(m1 > 0 && m1 < 2000000000LL, "number of band positions");
    SX_REQUIRE((row == nullptr) == (col == nullptr) && (row == nullptr) == (val == nullptr), "row, col and val come together");
    hipStream_t s = ctx->stream;
    const BmCsc csc = bm_csc(A);
    sx_stage tmp(ctx);
    int64_t *cnt = nullptr, *offs = nullptr;
    int *wid = nullptr;
    SX_TRY(tmp.tmp(static_cast<size_t>(m1), &cnt));
    SX_TRY(tmp.tmp(static_cast<size_t>(m1) + 1, &offs));
    SX_TRY(tmp.tmp(2, &wid));
    SX_HIP(hipMemsetAsync(wid, 0, 2 * sizeof(int), s));
    hipLaunchKernelGGL(k_bt_count, dim3(bm_grid(m1 * BM_G)), dim3(BM_WG), 0, s, m1, csc, bvar, rowb, cnt, wid);
    SX_TRY(sx_scan_exclusive(ctx, cnt, m1, offs));
    int64_t total = 0;
    int hw[2] = {0, 0};
    SX_HIP(hipMemcpyAsync(&total, offs + m1, sizeof(total), hipMemcpyDeviceToHost, s));
    SX_HIP(hipMemcpyAsync(hw, wid, sizeof(hw), hipMemcpyDeviceToHost, s));
    SX_HIP(hipStreamSynchronize(s));
    SX_HIP(hipGetLastError());
    if (count_host) *count_host = total;
    if (kl_host) *kl_host = hw[0];
    if (ku_host) *ku_host = hw[1];
    if (!row) return SX_OK;
    SX_REQUIRE(cap >= total, "room for %lld triplets, the band has %lld", (long long)cap, (long long)total);
    hipLaunchKernelGGL(k_bt_fill, dim3(bm_grid(m1 * BM_G)), dim3(BM_WG), 0, s, m1, csc, bvar, rowb, offs, row, col, val);
    SX_HIP(hipStreamSynchronize(s)); // (offs is freed on return)
    SX_HIP(hipGetLastError());
    return SX_OK;
}
