// Sparse crossover (kernel group K16s): from the point the first-order stage (sx_pdlp.hip) leaves -- or from a given
// basis -- to an optimal vertex and its basis WITHOUT a dense m x m inverse.  Stands where the reference's backends run
// their crossover behind the barrier (lp_methods/algorithms.py:50-54 -> solver_caller/gurobi.py:111-115) and their
// warm-started simplex (lp_methods/algorithms.py:69-74), all inside Gurobi.
//
// The design:
//   * the basis is factored in BORDERED form (sx_border.h): rows in their natural (or Cuthill-McKee) order, dense rows set
//     aside; every basic variable is matched to a band row by entry size -> B11, a band matrix (K16f); what finds no band
//     row -- the linking activities, logicals of dense rows -- forms the border together with the dense rows, and the
//     Schur complement of the border is factored by the dense LU (K16g).  EVERY basic variable is in the factors, so a
//     fresh factorisation of the current basis (full eta file, numerical trouble, final check) is a true
//     refactorisation, and a given basis (vbasis_in / cbasis_in) is taken as it is.  Columns the two LUs find
//     dependent leave the basis (superbasic), the logical of the row in question takes their place;
//   * the simplex works on an explicit TABLEAU of the few columns that can still move -- the superbasic ones plus what
//     pricing adds: T = B^-1 A_J (positions x |J|, column major in HBM, grown on demand).  A pivot is a ratio test down
//     one column, a copy of one row, and a rank-one update of T deferred in product form (64 per fold); every entering
//     column is also kept as an eta vector, so duals (B^-T c_B = B0^-T E_1^T .. E_k^T c_B) and new tableau columns
//     (E_k .. E_1 B0^-1 a_j) need no second factorisation until the eta file is full;
//   * when no tracked column prices out, all other columns are priced with those duals (the K1 walk) and the
//     violators join the tableau -- column generation, as in the reference's network crossover;
//   * before a vertex is called optimal its row residuals (one K2 walk) and the reduced costs of its basic columns are
//     checked against A itself; beyond the tolerances the basis is factored afresh and the run goes on.
// Memory O(nnz + m (kl + ku) + nb^2 + m |J|).  Everything that decides a pivot runs on the device; the host replays
// batches of pivots and reads one status word per batch.
//
// The file: kernels first; then the state of a call (HostLp, BandCall), of the basis (sx_plan::BasisState) and of one epoch
// (Epoch: device arrays, factors, border operators, tableau -- owned in one place); then one function per stage, and
// crossover_band_impl, which is the list of the stages and the three ways an epoch goes round again.  The host set-up
// between the device stages -- row order, matching, block geometry, triplets, the bookkeeping after the two LUs -- is
// sx_band_plan.h: plain C++ over vectors, tested on the CPU, and the seam a device-side set-up would replace.
#include "sx_internal.h"
#include "sx_border.h"
#include "sx_band_plan.h"

#include <algorithm>
#include <cstring>
#include <cmath>
#include <numeric>
#include <thread>

namespace {

constexpr int TB_WG = 256;
constexpr int TB_SUP = 3, TB_LOW = 1, TB_UPP = 2; // status of a tracked non-basic column
constexpr double TB_PIV = 1e-7;                   // smallest |alpha| the ratio test accepts
constexpr double TB_TINY = 1e-60; // band solves of tableau columns treat windows below this as zeros
constexpr double TB_DROP = 1e-14;                 // tableau entries below this become exact zeros (keeps B^-1 A_J local)

struct TbState {
    long long iters, max_iter, n_eta, cap_eta, pivots, flips, degen;
    int status;  // 0 running, 1 no tracked column prices out, 2 unbounded, 3 iteration limit, 4 numerical trouble
    int phase;   // 1: some basic variable is outside its bounds
    int q, dir;  // entering slot and its direction
    int r;       // leaving position (-1: bound flip of the entering column)
    int hit;     // bound the leaving variable stops at: 1 lower, 2 upper
    int n_inf;
    int n_bl;       // blocks of 256 positions in which the entering column has an entry (their list: blist)
    int n_pend;     // basis changes whose rank-one updates are not applied to T yet (product form: TbPend)
    int folding;    // the batch's fold is under way
    double theta, alpha_r, dq, sum_inf, feas_tol, opt_tol, tmax;
};

// Pending updates of a batch (product form).  Pivot s of the batch has entering slot q_s, leaving position r_s,
// u_s = alpha_s - e_{r_s} (alpha_s is the eta vector of the pivot) and v_s = row r_s of the tableau at that time
// divided by the pivot element (v_s[q_s] = 1 / pivot).  The current tableau column of slot j is
//     base_j - sum_{s >= s0[j]} u_s v_s[j],   base_j = T[:, j]  or  e_{sbase[j]} once j has been an entering slot,
// and row r is the same expression read across -- k vectors of m resp. |J| entries per pivot instead of a pass over
// the whole m x |J| tableau; k_tb_fold applies a batch in ONE pass (at 1e6 rows x 8,600 columns a rank-one update
// is 130 GB of traffic, 16 ms; the batch of 48-64 costs the same once).
constexpr int TB_K = 64;
struct TbPend {
    const double *vbuf; // [TB_K][ldv]
    const int32_t *pr;  // [TB_K] leaving position of the pending pivots
    const int32_t *s0;  // [slots] first pending pivot that applies to the slot
    const int32_t *sbase; // [slots] -1: base column is T's; >= 0: base column is that unit vector
    int64_t ldv;
};
__device__ __forceinline__ double tb_current(const double *__restrict__ T, const double *__restrict__ eta, const TbState *st,
                                              const TbPend &P, int64_t m, int64_t p, int j) {
    const int sb = P.sbase[j];
    double a = sb < 0 ? T[static_cast<size_t>(j) * m + p] : (p == sb ? 1.0 : 0.0);
    const int np = st->n_pend;
    const long long e0 = st->n_eta - np;
    for (int s = P.s0[j]; s < np; ++s) {
        const double u = eta[static_cast<size_t>(e0 + s) * m + p] - (p == P.pr[s] ? 1.0 : 0.0);
        a -= u * P.vbuf[static_cast<size_t>(s) * P.ldv + j];
    }
    return a;
}

struct TbPart {
    double t, a;
    int p, hit;
};

// ---------------------------------------------------------------------------------------------- set-up kernels
__global__ __launch_bounds__(TB_WG) void k_tb_scatter_cols(int64_t nslots, const int32_t *__restrict__ var, int64_t n,
                                                           const int64_t *__restrict__ cptr, const int32_t *__restrict__ cidx,
                                                           const double *__restrict__ cval, const int32_t *__restrict__ eqidx,
                                                           double *__restrict__ T, int64_t m) {
    const int64_t s = static_cast<int64_t>(blockIdx.x) * TB_WG + threadIdx.x;
    if (s >= nslots) return;
    double *col = T + static_cast<size_t>(s) * m;
    const int64_t v = var[s];
    if (v >= n) {
        col[eqidx[v - n]] = 1.0;
        return;
    }
    for (int64_t k = cptr[v]; k < cptr[v + 1]; ++k) col[eqidx[cidx[k]]] = cval[k];
}

__device__ __forceinline__ double tb_block_sum(double v, double *sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = ((sm[0] + sm[1]) + sm[2]) + sm[3];
    __syncthreads();
    return r;
}

// The probe's short cut: out[0] = the tallest column of A over the rows that are not dense (largest - smallest row index of
// a column's entries in such rows), out[1] = the number of dense rows.  Whatever columns a basis takes and whatever rows they
// are matched to, an entry lies at most that far from its column's position in the natural order of the band rows (setting
// rows aside only shortens distances): kl, ku <= out[0].
__global__ __launch_bounds__(TB_WG) void k_tb_colspan(int64_t m, int64_t n, const int64_t *__restrict__ cptr, const int32_t *__restrict__ cidx,
                                                      const int64_t *__restrict__ rptr, int64_t dense_thr, int *__restrict__ out) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * TB_WG + threadIdx.x;
    int span = 0, dense = 0;
    if (t < n) {
        int lo = INT32_MAX, hi = -1;
        for (int64_t k = cptr[t]; k < cptr[t + 1]; ++k) {
            const int i = cidx[k];
            if (rptr[i + 1] - rptr[i] > dense_thr) continue;
            lo = i < lo ? i : lo;
            hi = i > hi ? i : hi;
        }
        if (hi >= 0) span = hi - lo;
    }
    if (t < m && rptr[t + 1] - rptr[t] > dense_thr) dense = 1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(span, o, 64);
        span = other > span ? other : span;
        dense += __shfl_xor(dense, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (span > 0) atomicMax(&out[0], span);
        if (dense > 0) atomicAdd(&out[1], dense);
    }
}

// dst[:, dest[s]] = src[:, s]  (rows x gridDim.y columns)
__global__ __launch_bounds__(TB_WG) void k_tb_copy_cols(int64_t rows, const double *__restrict__ src, int64_t lds_, const int32_t *__restrict__ dest,
                                                        double *__restrict__ dst, int64_t ldd) {
    const int64_t sc = blockIdx.y;
    const double *a = src + static_cast<size_t>(sc) * lds_;
    double *o = dst + static_cast<size_t>(dest[sc]) * ldd;
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * TB_WG + threadIdx.x; r < rows; r += static_cast<int64_t>(gridDim.x) * TB_WG) o[r] = a[r];
}

// entries below the drop tolerance -> exact zeros (what the pivots skip)
// (grid-stride: a launch carries fewer than 2^32 work-items, a tableau has more entries than that)
__global__ __launch_bounds__(TB_WG) void k_tb_drop(int64_t total, double *__restrict__ W, double tol) {
    for (int64_t t = static_cast<int64_t>(blockIdx.x) * TB_WG + threadIdx.x; t < total; t += static_cast<int64_t>(gridDim.x) * TB_WG)
        if (fabs(W[t]) < tol) W[t] = 0.0;
}

// out[s] = base[s] - sum_p w[p] T[p, s]        (one workgroup per tracked column)
__global__ __launch_bounds__(TB_WG) void k_tb_coldot(int64_t m, const double *__restrict__ T, const double *__restrict__ w,
                                                      const double *__restrict__ base, double *__restrict__ out) {
    __shared__ double sm[4];
    const int64_t s = blockIdx.x;
    const double *col = T + static_cast<size_t>(s) * m;
    double acc = 0.0;
    for (int64_t p = threadIdx.x; p < m; p += TB_WG) {
        const double t = col[p];
        if (t != 0.0) acc += w[p] * t;
    }
    const double tot = tb_block_sum(acc, sm);
    if (threadIdx.x == 0) out[s] = (base ? base[s] : 0.0) - tot;
}

// ---------------------------------------------------------------------------------------------- one pivot
// infeasibility signs of the basic variables; per-workgroup counts
__global__ __launch_bounds__(TB_WG) void k_tb_infeas(int64_t m, const double *__restrict__ xB, const double *__restrict__ lB,
                                                     const double *__restrict__ uB, const TbState *__restrict__ st,
                                                     double *__restrict__ g, double *__restrict__ part) {
    __shared__ double sm[4];
    if (st->status != 0) return;
    const int64_t p = static_cast<int64_t>(blockIdx.x) * TB_WG + threadIdx.x;
    double gi = 0.0, inf = 0.0;
    if (p < m) {
        const double x = xB[p], tol = st->feas_tol;
        if (x > uB[p] + tol) {
            gi = 1.0;
            inf = x - uB[p];
        } else if (x < lB[p] - tol) {
            gi = -1.0;
            inf = lB[p] - x;
        }
        g[p] = gi;
    }
    const double cnt = tb_block_sum(gi != 0.0 ? 1.0 : 0.0, sm);
    const double sum = tb_block_sum(inf, sm);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = cnt;
        part[2 * blockIdx.x + 1] = sum;
    }
}

__global__ __launch_bounds__(TB_WG) void k_tb_phase(int nblk, const double *__restrict__ part, TbState *st, int32_t *__restrict__ infoff) {
    __shared__ double sm[4];
    __shared__ int sc[TB_WG];
    if (st->status != 0) return;
    // thread t owns the blocks [t c, (t + 1) c): their counts, then an exclusive scan -> infoff[block] = infeasible
    // positions before it (k_tb_inflist writes the list of positions in ascending order from these)
    const int chunk = (nblk + TB_WG - 1) / TB_WG;
    const int k0 = threadIdx.x * chunk, k1 = (k0 + chunk < nblk) ? k0 + chunk : nblk;
    double cnt = 0.0, sum = 0.0;
    for (int k = k0; k < k1; ++k) { // (counts are small integers: any order gives the same sum)
        cnt += part[2 * k];
        sum += part[2 * k + 1];
    }
    const int mine = static_cast<int>(cnt);
    sc[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 1; o < TB_WG; o <<= 1) {
        const int v = (threadIdx.x >= o) ? sc[threadIdx.x - o] : 0;
        __syncthreads();
        sc[threadIdx.x] += v;
        __syncthreads();
    }
    int run = sc[threadIdx.x] - mine;
    for (int k = k0; k < k1; ++k) {
        infoff[k] = run;
        run += static_cast<int>(part[2 * k]);
    }
    cnt = tb_block_sum(cnt, sm);
    sum = tb_block_sum(sum, sm);
    if (threadIdx.x == 0) {
        st->n_inf = static_cast<int>(cnt);
        st->sum_inf = sum;
        st->phase = cnt > 0.0 ? 1 : 2;
    }
}

// phase 1: the infeasible positions in ascending order (at most TB_INFLIST of them; more: the pricing kernels read
// the columns whole).  A workgroup per block of 256 positions that holds one: ordered compaction by ballots.
constexpr int TB_INFLIST = 4096;
__global__ __launch_bounds__(TB_WG) void k_tb_inflist(int64_t m, const double *__restrict__ g, const double *__restrict__ part,
                                                      const int32_t *__restrict__ infoff, const TbState *__restrict__ st,
                                                      int32_t *__restrict__ list) {
    __shared__ int wsum[TB_WG / 64];
    if (st->status != 0 || st->phase != 1 || st->n_inf > TB_INFLIST) return;
    if (part[2 * blockIdx.x] <= 0.0) return;
    const int64_t p = static_cast<int64_t>(blockIdx.x) * TB_WG + threadIdx.x;
    const bool hit = p < m && g[p] != 0.0;
    const unsigned long long bal = __ballot(hit);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    if (hit) list[infoff[blockIdx.x] + before + __popcll(bal & ((1ull << lane) - 1ull))] = static_cast<int32_t>(p);
}

// phase 1 only: d1[j] = - g^T (current column j) = -( g^T base_j - sum_{s >= s0[j]} (g^T u_s) v_s[j] ).  Few basic
// variables are infeasible behind a first-order point, so g^T T[:, j] gathers the listed positions only (k_tb_inflist:
// ~200 of 1e6 at config-5 size -- scanning the 256-position blocks that hold one cost 1.3 ms per iteration there);
// with more than TB_INFLIST of them it reads the column whole, coalesced.
__global__ __launch_bounds__(TB_WG) void k_tb_gu(int64_t m, int nblk, const double *__restrict__ eta, const double *__restrict__ g,
                                                 const int32_t *__restrict__ list, const TbState *__restrict__ st, TbPend P,
                                                 double *__restrict__ gu) {
    __shared__ double sm[4];
    if (st->status != 0 || st->phase != 1) return;
    const int sidx = blockIdx.x;
    if (sidx >= st->n_pend) return;
    const double *al = eta + static_cast<size_t>(st->n_eta - st->n_pend + sidx) * m;
    const int r = P.pr[sidx];
    double acc = 0.0;
    if (st->n_inf <= TB_INFLIST) {
        for (int i = threadIdx.x; i < st->n_inf; i += TB_WG) {
            const int p = list[i];
            acc += g[p] * (al[p] - (p == r ? 1.0 : 0.0));
        }
    } else {
        for (int64_t p = threadIdx.x; p < m; p += TB_WG) {
            const double gp = g[p];
            if (gp != 0.0) acc += gp * (al[p] - (p == r ? 1.0 : 0.0));
        }
    }
    const double tot = tb_block_sum(acc, sm);
    if (threadIdx.x == 0) gu[sidx] = tot;
}

__global__ __launch_bounds__(TB_WG) void k_tb_price1(int64_t m, int nblk, const double *__restrict__ T, const double *__restrict__ g,
                                                     const int32_t *__restrict__ list, const TbState *__restrict__ st, TbPend P,
                                                     const double *__restrict__ gu, double *__restrict__ d1) {
    __shared__ double sm[4];
    if (st->status != 0 || st->phase != 1) return;
    const int64_t s = blockIdx.x;
    const int sb = P.sbase[s];
    double acc = 0.0;
    if (sb >= 0) {
        if (threadIdx.x == 0) acc = g[sb];
    } else {
        const double *col = T + static_cast<size_t>(s) * m;
        if (st->n_inf <= TB_INFLIST) {
            for (int i = threadIdx.x; i < st->n_inf; i += TB_WG) {
                const int p = list[i];
                acc += g[p] * col[p];
            }
        } else {
            for (int64_t p = threadIdx.x; p < m; p += TB_WG) {
                const double gp = g[p];
                if (gp != 0.0) acc += gp * col[p];
            }
        }
    }
    double tot = tb_block_sum(acc, sm);
    if (threadIdx.x == 0) {
        for (int k = P.s0[s]; k < st->n_pend; ++k) tot -= gu[k] * P.vbuf[static_cast<size_t>(k) * P.ldv + s];
        d1[s] = -tot;
    }
}

// entering column: superbasic columns first (they have to leave their interior value), then the largest
// reduced cost of the right sign; one workgroup
__global__ __launch_bounds__(TB_WG) void k_tb_select(int64_t nJ, const double *__restrict__ dJ, const double *__restrict__ d1,
                                                     const int32_t *__restrict__ statJ, const double *__restrict__ xJ,
                                                     const double *__restrict__ lJ, const double *__restrict__ uJ, TbState *st) {
    __shared__ double bv[TB_WG];
    __shared__ int bi[TB_WG], bd[TB_WG];
    if (st->status != 0) return;
    const bool ph1 = st->phase == 1;
    const double tol = st->opt_tol;
    double best = -1.0;
    int bs = -1, bdir = 0;
    for (int64_t s = threadIdx.x; s < nJ; s += TB_WG) {
        const int stt = statJ[s];
        if (stt == 0) continue; // empty slot
        const double d = ph1 ? d1[s] : dJ[s];
        double score = -1.0;
        int dir = 0;
        const bool fixed = lJ[s] == uJ[s];
        if (fixed && stt != TB_SUP) continue;
        if (stt == TB_SUP) {
            if (d < -tol) dir = 1;
            else if (d > tol) dir = -1;
            if (dir != 0) score = fabs(d) + 1e30; // a superbasic column that prices out: first of all
            else if (!ph1) {
                // prices at zero: still has to reach a bound (vertex); towards the nearer one
                const double dl = xJ[s] - lJ[s], du = uJ[s] - xJ[s];
                if (!(isinf(dl) && isinf(du))) {
                    dir = (dl <= du) ? -1 : 1;
                    score = 1e29;
                }
            }
        } else if (stt == TB_LOW) {
            if (d < -tol) {
                dir = 1;
                score = -d;
            }
        } else if (stt == TB_UPP) {
            if (d > tol) {
                dir = -1;
                score = d;
            }
        }
        if (score > best) {
            best = score;
            bs = static_cast<int>(s);
            bdir = dir;
        }
    }
    bv[threadIdx.x] = best;
    bi[threadIdx.x] = bs;
    bd[threadIdx.x] = bdir;
    __syncthreads();
    for (int o = TB_WG / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            const double ob = bv[threadIdx.x + o];
            const int oi = bi[threadIdx.x + o];
            if (ob > bv[threadIdx.x] || (ob == bv[threadIdx.x] && oi >= 0 && (bi[threadIdx.x] < 0 || oi < bi[threadIdx.x]))) {
                bv[threadIdx.x] = ob;
                bi[threadIdx.x] = oi;
                bd[threadIdx.x] = bd[threadIdx.x + o];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (bi[0] < 0) {
            st->status = 1; // nothing tracked prices out (in phase 1: with respect to the infeasibility)
            st->q = -1;
        } else {
            st->q = bi[0];
            st->dir = bd[0];
            st->dq = dJ[bi[0]];
            if (st->iters >= st->max_iter) st->status = 3;
            else if (st->n_eta >= st->cap_eta) st->status = 3;
        }
    }
}

// Ratio test down the entering column (Harris, two passes): pass 1 finds the longest step that keeps every basic
// variable within feas_tol of its bounds; pass 2 takes, among the rows that block no later than that, the one with
// the largest pivot.  The column is kept as the eta vector of this pivot.
__device__ __forceinline__ void tb_row_limit(double a, double dir, double x, double lo, double up, double tol, double &dist, double &rate,
                                             int &hit) {
    // distance of x_B[p] to the bound it moves towards (inf: none) and |rate| of the approach
    rate = fabs(a);
    hit = 0;
    dist = INFINITY;
    const double r = -dir * a;
    if (r < 0.0) {
        if (x > up + tol) { // starts above its upper bound: becomes feasible there
            dist = x - up;
            hit = 2;
        } else if (!isinf(lo) && x >= lo - tol) {
            dist = fmax(x - lo, 0.0);
            hit = 1;
        }
    } else {
        if (x < lo - tol) {
            dist = lo - x;
            hit = 1;
        } else if (!isinf(up) && x <= up + tol) {
            dist = fmax(up - x, 0.0);
            hit = 2;
        }
    }
}

__global__ __launch_bounds__(TB_WG) void k_tb_ratio1(int64_t m, const double *__restrict__ T, const double *__restrict__ xB,
                                                     const double *__restrict__ lB, const double *__restrict__ uB,
                                                     const TbState *__restrict__ st, double *__restrict__ eta,
                                                     double *__restrict__ part, TbPend P) {
    __shared__ double sm[TB_WG];
    __shared__ int any_nz;
    if (st->status != 0) return;
    if (threadIdx.x == 0) any_nz = 0;
    __syncthreads();
    const int64_t p = static_cast<int64_t>(blockIdx.x) * TB_WG + threadIdx.x;
    const double dir = static_cast<double>(st->dir), tol = st->feas_tol;
    double t = INFINITY;
    if (p < m) {
        double a = tb_current(T, eta, st, P, m, p, st->q);
        if (fabs(a) < TB_DROP) a = 0.0;
        eta[static_cast<size_t>(st->n_eta) * m + p] = a;
        if (a != 0.0) any_nz = 1; // (benign race: every writer stores 1)
        if (fabs(a) > TB_PIV) {
            double dist, rate;
            int hit;
            tb_row_limit(a, dir, xB[p], lB[p], uB[p], tol, dist, rate, hit);
            if (hit) t = (dist + tol) / rate;
        }
    }
    sm[threadIdx.x] = t;
    __syncthreads();
    for (int o = TB_WG / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) sm[threadIdx.x] = fmin(sm[threadIdx.x], sm[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[blockIdx.x] = sm[0];
        part[gridDim.x + blockIdx.x] = any_nz ? 1.0 : 0.0;
    }
}

__global__ __launch_bounds__(TB_WG) void k_tb_tmax(int nblk, const double *__restrict__ part, TbState *st, int32_t *__restrict__ blist) {
    __shared__ double sm[TB_WG];
    __shared__ int cnt[TB_WG];
    if (st->status != 0) return;
    // every lane a contiguous run of blocks: the list comes out in ascending order whatever the run lengths
    const int per = (nblk + TB_WG - 1) / TB_WG;
    const int k0 = threadIdx.x * per, k1 = (k0 + per < nblk) ? k0 + per : nblk;
    double t = INFINITY;
    int mine = 0;
    for (int k = k0; k < k1; ++k) {
        t = fmin(t, part[k]);
        if (part[nblk + k] != 0.0) ++mine;
    }
    sm[threadIdx.x] = t;
    cnt[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tm = INFINITY;
        int run = 0;
        for (int w = 0; w < TB_WG; ++w) {
            tm = fmin(tm, sm[w]);
            const int c = cnt[w];
            cnt[w] = run;
            run += c;
        }
        st->tmax = tm;
        st->n_bl = run;
    }
    __syncthreads();
    int o = cnt[threadIdx.x];
    for (int k = k0; k < k1; ++k)
        if (part[nblk + k] != 0.0) blist[o++] = k;
}

__global__ __launch_bounds__(TB_WG) void k_tb_ratio(int64_t m, const double *__restrict__ xB, const double *__restrict__ lB,
                                                    const double *__restrict__ uB, const TbState *__restrict__ st,
                                                    const double *__restrict__ eta, TbPart *__restrict__ part) {
    __shared__ double st_[TB_WG], sa_[TB_WG];
    __shared__ int sp_[TB_WG], sh_[TB_WG];
    if (st->status != 0) return;
    const int64_t p = static_cast<int64_t>(blockIdx.x) * TB_WG + threadIdx.x;
    const double dir = static_cast<double>(st->dir), tol = st->feas_tol, tmax = st->tmax;
    double t = INFINITY, aa = -1.0;
    int hit = 0;
    if (p < m) {
        const double a = eta[static_cast<size_t>(st->n_eta) * m + p];
        if (fabs(a) > TB_PIV) {
            double dist, rate;
            int h;
            tb_row_limit(a, dir, xB[p], lB[p], uB[p], tol, dist, rate, h);
            if (h && dist / rate <= tmax) {
                t = dist / rate;
                aa = rate;
                hit = h;
            }
        }
    }
    st_[threadIdx.x] = t;
    sa_[threadIdx.x] = aa;
    sp_[threadIdx.x] = static_cast<int>(p);
    sh_[threadIdx.x] = hit;
    __syncthreads();
    for (int o = TB_WG / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            if (sa_[threadIdx.x + o] > sa_[threadIdx.x]) { // larger pivot; ties to the smaller position (kept)
                st_[threadIdx.x] = st_[threadIdx.x + o];
                sa_[threadIdx.x] = sa_[threadIdx.x + o];
                sp_[threadIdx.x] = sp_[threadIdx.x + o];
                sh_[threadIdx.x] = sh_[threadIdx.x + o];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        TbPart r;
        r.t = st_[0];
        r.a = sa_[0];
        r.p = sp_[0];
        r.hit = sh_[0];
        part[blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(TB_WG) void k_tb_decide(int nblk, const TbPart *__restrict__ part, const double *__restrict__ xJ,
                                                     const double *__restrict__ lJ, const double *__restrict__ uJ,
                                                     const int32_t *__restrict__ statJ, TbState *st) {
    __shared__ double sa_[TB_WG], st_[TB_WG];
    __shared__ int sp_[TB_WG], sh_[TB_WG];
    if (st->status != 0) return;
    // largest pivot among the rows pass 2 admitted; ties to the smaller position (blocks are in position order)
    TbPart b;
    b.a = -1.0;
    b.t = INFINITY;
    b.p = 0x7fffffff;
    b.hit = 0;
    for (int k = threadIdx.x; k < nblk; k += TB_WG) {
        const TbPart o = part[k];
        if (o.a > b.a || (o.a == b.a && o.p < b.p)) b = o;
    }
    sa_[threadIdx.x] = b.a;
    st_[threadIdx.x] = b.t;
    sp_[threadIdx.x] = b.p;
    sh_[threadIdx.x] = b.hit;
    __syncthreads();
    for (int o = TB_WG / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            const int j = threadIdx.x + o;
            if (sa_[j] > sa_[threadIdx.x] || (sa_[j] == sa_[threadIdx.x] && sp_[j] < sp_[threadIdx.x])) {
                sa_[threadIdx.x] = sa_[j];
                st_[threadIdx.x] = st_[j];
                sp_[threadIdx.x] = sp_[j];
                sh_[threadIdx.x] = sh_[j];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    b.a = sa_[0];
    b.t = st_[0];
    b.p = sp_[0];
    b.hit = sh_[0];
    if (b.a < 0.0) b.t = INFINITY; // no row blocks
    const int q = st->q;
    // the entering column's own way to its other bound
    double own = INFINITY;
    if (st->dir > 0) own = uJ[q] - xJ[q];
    else own = xJ[q] - lJ[q];
    if (own < 0.0) own = 0.0;
    if (isinf(b.t) && isinf(own)) {
        st->status = st->phase == 1 ? 4 : 2;
        return;
    }
    if (own <= b.t) {
        st->r = -1;
        st->theta = own;
        st->hit = st->dir > 0 ? 2 : 1;
    } else {
        st->r = b.p;
        st->theta = b.t;
        st->hit = b.hit;
    }
}

// row r of the current tableau -> rowbuf; alpha_r
__global__ __launch_bounds__(TB_WG) void k_tb_rowcopy(int64_t m, int64_t nJ, const double *__restrict__ T, const double *__restrict__ eta,
                                                      TbState *st, TbPend P, double *__restrict__ rowbuf) {
    if (st->status != 0 || st->r < 0) return;
    const int64_t s = static_cast<int64_t>(blockIdx.x) * TB_WG + threadIdx.x;
    if (s >= nJ) return;
    double v = tb_current(T, eta, st, P, m, st->r, static_cast<int>(s));
    if (fabs(v) < TB_DROP) v = 0.0;
    if (s == st->q) {
        v = eta[static_cast<size_t>(st->n_eta) * m + st->r]; // (the very number the ratio test saw)
        st->alpha_r = v;
    }
    rowbuf[s] = v;
}

// x_B moves along the entering column (only the blocks of positions in which that column has an entry); the
// tableau itself is not touched: the pivot joins the pending batch (k_tb_post) and k_tb_fold applies the batch
__global__ __launch_bounds__(TB_WG) void k_tb_update(int64_t m, double *__restrict__ xB, const double *__restrict__ eta,
                                                     const TbState *__restrict__ st, const int32_t *__restrict__ blist) {
    if (st->status != 0) return;
    const int r = st->r;
    for (int e = blockIdx.x; e < st->n_bl; e += gridDim.x) {
        const int64_t p = static_cast<int64_t>(blist[e]) * TB_WG + threadIdx.x;
        if (p >= m || p == r) continue;
        const double a = eta[static_cast<size_t>(st->n_eta) * m + p];
        if (a != 0.0) xB[p] = xB[p] - static_cast<double>(st->dir) * st->theta * a;
    }
}

// One pass over the tableau for a whole batch: T[p, j] = base - sum_{s >= s0[j]} u_s[p] v_s[j].  A lane owns a
// position (its u_s in registers, 64 at most), a workgroup TB_FJ slots (their v_s in LDS).
__global__ void k_tb_fold_begin(TbState *st, int slack) {
    st->folding = (st->n_pend > 0 && (st->status != 0 || st->n_pend + slack > TB_K)) ? 1 : 0;
}
constexpr int TB_FJ = 64; // slots per workgroup of the fold: the batch's u_s[p] are read once per TB_FJ columns
__global__ __launch_bounds__(TB_WG) void k_tb_fold(int64_t m, int64_t nJ, double *__restrict__ T, const double *__restrict__ eta,
                                                   const TbState *__restrict__ st, TbPend P) {
    __shared__ double vs[TB_K][TB_FJ + 1];
    __shared__ int ss0[TB_FJ], ssb[TB_FJ], snz[TB_FJ];
    if (!st->folding) return;
    const int np = st->n_pend;
    const long long e0 = st->n_eta - np;
    const int64_t j0 = static_cast<int64_t>(blockIdx.y) * TB_FJ;
    const int nj = static_cast<int>((nJ - j0 < TB_FJ) ? nJ - j0 : TB_FJ);
    if (threadIdx.x < TB_FJ) {
        ss0[threadIdx.x] = threadIdx.x < nj ? P.s0[j0 + threadIdx.x] : np;
        ssb[threadIdx.x] = threadIdx.x < nj ? P.sbase[j0 + threadIdx.x] : -1;
        snz[threadIdx.x] = 0;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < TB_K * TB_FJ; e += TB_WG) {
        const int sidx = e / TB_FJ, jj = e % TB_FJ;
        // zero where the pivot does not apply to the slot (before its s0, beyond the batch): the inner loop below is 64
        // multiply-adds without a test -- with `if (sidx >= first && sidx < np)` around each, the uniform branches cost five
        // times the arithmetic (105 ms per pass at config-5 size)
        const double v = (sidx < np && jj < nj && sidx >= ss0[jj]) ? P.vbuf[static_cast<size_t>(sidx) * P.ldv + j0 + jj] : 0.0;
        vs[sidx][jj] = v;
        if (v != 0.0) snz[jj] = 1; // (every writer stores 1)
    }
    __syncthreads();
    for (int64_t p = static_cast<int64_t>(blockIdx.x) * TB_WG + threadIdx.x; p < m; p += static_cast<int64_t>(gridDim.x) * TB_WG) {
        double u[TB_K];
        bool any = false;
#pragma unroll
        for (int sidx = 0; sidx < TB_K; ++sidx) {
            double x = 0.0;
            if (sidx < np) x = eta[static_cast<size_t>(e0 + sidx) * m + p] - (p == P.pr[sidx] ? 1.0 : 0.0);
            u[sidx] = x;
            any = any || x != 0.0;
        }
        for (int jj = 0; jj < nj; ++jj) {
            const int sb = ssb[jj];
            // the row saw none of the batch's pivots, or the column none of its pivot rows: the slot keeps its entry
            if ((!any || !snz[jj]) && sb < 0) continue;
            double *t = T + static_cast<size_t>(j0 + jj) * m + p;
            double acc = sb < 0 ? *t : (p == sb ? 1.0 : 0.0);
#pragma unroll
            for (int sidx = 0; sidx < TB_K; ++sidx) acc = __builtin_fma(-u[sidx], vs[sidx][jj], acc); // (u is zero beyond the batch)
            *t = fabs(acc) < TB_DROP ? 0.0 : acc;
        }
    }
}
__global__ __launch_bounds__(TB_WG) void k_tb_fold_end(int64_t nJ, TbState *st, int32_t *__restrict__ s0, int32_t *__restrict__ sbase) {
    if (!st->folding) return;
    const int64_t j = static_cast<int64_t>(blockIdx.x) * TB_WG + threadIdx.x;
    if (j < nJ) {
        s0[j] = 0;
        sbase[j] = -1;
    }
}
__global__ void k_tb_fold_done(TbState *st) {
    if (st->folding) {
        st->n_pend = 0;
        st->folding = 0;
    }
}

// reduced costs of the tracked columns and the bookkeeping of the pivot; one workgroup
__global__ __launch_bounds__(TB_WG) void k_tb_post(int64_t nJ, double *__restrict__ dJ, const double *__restrict__ rowbuf,
                                                   int32_t *__restrict__ head, double *__restrict__ xB, double *__restrict__ lB,
                                                   double *__restrict__ uB, double *__restrict__ cB, int32_t *__restrict__ varJ,
                                                   double *__restrict__ xJ, double *__restrict__ lJ, double *__restrict__ uJ,
                                                   double *__restrict__ cJ, int32_t *__restrict__ statJ, int32_t *__restrict__ eta_r,
                                                   TbState *st, double *__restrict__ vbuf, int64_t ldv, int32_t *__restrict__ pr,
                                                   int32_t *__restrict__ s0, int32_t *__restrict__ sbase) {
    if (st->status != 0) return;
    const int q = st->q, r = st->r;
    const double dq = st->dq, ar = st->alpha_r;
    if (r >= 0) {
        const double f = dq / ar;
        const bool good = fabs(ar) > TB_PIV;
        double *v = vbuf + static_cast<size_t>(st->n_pend) * ldv;
        for (int64_t s = threadIdx.x; s < nJ; s += TB_WG) {
            const double rb = rowbuf[s];
            if (s != q) {
                if (rb != 0.0) dJ[s] = dJ[s] - f * rb;
                if (good) v[s] = rb / ar;
            } else if (good) {
                v[s] = 1.0 / ar;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double xq = xJ[q] + static_cast<double>(st->dir) * st->theta;
    st->iters += 1;
    if (!(st->theta > 1e-12)) st->degen += 1;
    if (r < 0) { // the entering column went to its other bound
        xJ[q] = st->hit == 2 ? uJ[q] : lJ[q];
        statJ[q] = st->hit == 2 ? TB_UPP : TB_LOW;
        st->flips += 1;
        return;
    }
    if (!(fabs(ar) > TB_PIV)) {
        st->status = 4;
        return;
    }
    // leaving variable -> slot q at the bound it hit; entering variable -> position r
    const int32_t vout = head[r];
    const double lo = lB[r], up = uB[r], co = cB[r];
    head[r] = varJ[q];
    xB[r] = xq;
    lB[r] = lJ[q];
    uB[r] = uJ[q];
    cB[r] = cJ[q];
    varJ[q] = vout;
    lJ[q] = lo;
    uJ[q] = up;
    cJ[q] = co;
    xJ[q] = st->hit == 2 ? up : lo;
    statJ[q] = st->hit == 2 ? TB_UPP : TB_LOW;
    dJ[q] = -dq / ar;
    eta_r[st->n_eta] = r;
    pr[st->n_pend] = r;
    s0[q] = st->n_pend; // the slot now holds the leaving variable: its column is e_r - u v[q] from this pivot on
    sbase[q] = r;
    st->n_pend += 1;
    st->n_eta += 1;
    st->pivots += 1;
}

// ---------------------------------------------------------------------------------------------- eta file
// W <- E_{k0+K-1} ... E_{k0} W for ncols columns (ldw = m), K <= TB_EB etas at a time.  One eta: w_r <- w_r / alpha_r,
// w_p <- w_p - alpha_p w_r (p != r), i.e. w <- w - u sigma with u = alpha - e_r and sigma = w_r / alpha_r.  K of them:
// sigma_i = (w0[r_i] - sum_{j<i} u_j[r_i] sigma_j) / alpha_i[r_i] (a K x K triangle per column), then W <- W - U Sigma in
// ONE pass over W instead of K (applying 8,214 etas to 373 columns one eta at a time moved 9 GB per eta: 16.5 s).
constexpr int TB_EB = 64; // etas per block
constexpr int TB_EC = 64; // columns per workgroup of the rank-K pass (16: the eta block was re-read once per 16 columns -- 12 GB of a 18 GB pass at 1e6 rows x 373 columns)
__global__ __launch_bounds__(TB_WG) void k_tb_etab_gather(int64_t m, int64_t ncols, const double *__restrict__ W, const double *__restrict__ eta,
                                                          const int32_t *__restrict__ eta_r, int64_t k0, int K, double *__restrict__ G,
                                                          double *__restrict__ M) {
    // G[i][c] = W[r_i, c];  M[i][j] = u_j[r_i] (j < i), M[i][i] = alpha_i[r_i]
    const int64_t t = static_cast<int64_t>(blockIdx.x) * TB_WG + threadIdx.x;
    if (t < static_cast<int64_t>(TB_EB) * ncols) {
        const int i = static_cast<int>(t / ncols);
        const int64_t c = t - static_cast<int64_t>(i) * ncols;
        G[t] = (i < K) ? W[static_cast<size_t>(c) * m + eta_r[k0 + i]] : 0.0;
    }
    if (t < TB_EB * TB_EB) {
        const int i = static_cast<int>(t) / TB_EB, j = static_cast<int>(t) % TB_EB;
        double v = (i == j) ? 1.0 : 0.0;
        if (i < K && j <= i) {
            const int ri = eta_r[k0 + i];
            v = eta[static_cast<size_t>(k0 + j) * m + ri];
            if (j < i && eta_r[k0 + j] == ri) v -= 1.0;
        }
        M[t] = v;
    }
}
__global__ __launch_bounds__(64) void k_tb_etab_solve(int64_t ncols, const double *__restrict__ G, const double *__restrict__ M,
                                                      double *__restrict__ S, int32_t *__restrict__ colflag) {
    __shared__ double sM[TB_EB * TB_EB];
    for (int e = threadIdx.x; e < TB_EB * TB_EB; e += 64) sM[e] = M[e];
    __syncthreads();
    const int64_t c = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;
    if (c >= ncols) return;
    double sg[TB_EB];
    int any = 0;
#pragma unroll
    for (int i = 0; i < TB_EB; ++i) {
        double x = G[static_cast<size_t>(i) * ncols + c];
#pragma unroll
        for (int j = 0; j < i; ++j) x -= sM[i * TB_EB + j] * sg[j];
        sg[i] = x / sM[i * TB_EB + i];
        any |= sg[i] != 0.0;
    }
#pragma unroll
    for (int i = 0; i < TB_EB; ++i) S[static_cast<size_t>(i) * ncols + c] = sg[i];
    colflag[c] = any;
}
__global__ __launch_bounds__(TB_WG) void k_tb_etab_apply(int64_t m, int64_t ncols, double *__restrict__ W, const double *__restrict__ eta,
                                                         const int32_t *__restrict__ eta_r, int64_t k0, int K, const double *__restrict__ S,
                                                         const int32_t *__restrict__ colflag) {
    __shared__ double sS[TB_EB * TB_EC];
    __shared__ int sflag[TB_EC], sr[TB_EB], sany;
    const int64_t c0 = static_cast<int64_t>(blockIdx.y) * TB_EC;
    const int nc = static_cast<int>((ncols - c0 < TB_EC) ? ncols - c0 : TB_EC);
    if (threadIdx.x == 0) sany = 0;
    __syncthreads();
    if (threadIdx.x < TB_EC) {
        const int fl = (threadIdx.x < nc) ? colflag[c0 + threadIdx.x] : 0;
        sflag[threadIdx.x] = fl;
        if (fl) sany = 1;
    }
    if (threadIdx.x < TB_EB) sr[threadIdx.x] = (threadIdx.x < K) ? eta_r[k0 + threadIdx.x] : -1;
    for (int e = threadIdx.x; e < TB_EB * TB_EC; e += TB_WG) {
        const int i = e / TB_EC, cc = e % TB_EC;
        sS[e] = (cc < nc) ? S[static_cast<size_t>(i) * ncols + c0 + cc] : 0.0;
    }
    __syncthreads();
    if (!sany) return; // none of the tile's columns meets a pivot row of the block
    for (int64_t p = static_cast<int64_t>(blockIdx.x) * TB_WG + threadIdx.x; p < m; p += static_cast<int64_t>(gridDim.x) * TB_WG) {
        double u[TB_EB];
        int nz = 0;
#pragma unroll
        for (int i = 0; i < TB_EB; ++i) {
            double a = (i < K) ? eta[static_cast<size_t>(k0 + i) * m + p] : 0.0;
            if (sr[i] == p) a -= 1.0;
            u[i] = a;
            nz |= a != 0.0;
        }
        if (!nz) continue;
        for (int cc = 0; cc < nc; ++cc) {
            if (!sflag[cc]) continue;
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < TB_EB; ++i) acc += u[i] * sS[i * TB_EC + cc];
            double *w = W + static_cast<size_t>(c0 + cc) * m + p;
            *w = *w - acc;
        }
    }
}
// v <- E_{k0}^T ... E_{k0+K-1}^T v (the duals' way through the eta file: the youngest eta first), K <= TB_EB etas per pass.
// One eta: v[r] <- (v[r] - sum_{p != r} alpha[p] v[p]) / alpha[r]: a dot over all positions that changes ONE entry, so the K dots
// of a block are taken against the vector the block found (k_tb_etat_dots: one pass over the K eta columns, all workgroups busy)
// and corrected by what the younger etas of the block changed -- a K x K triangle in one wave (k_tb_etat_solve).  One eta at a
// time this was 2 launches and a 64-workgroup dot per eta: 80 ms per pricing round with 921 etas over 1e6 positions.
constexpr int TB_ETS = 32; // slices of the positions per eta column (partial dots, summed in order)
__global__ __launch_bounds__(TB_WG) void k_tb_etat_dots(int64_t m, const double *__restrict__ v, const double *__restrict__ eta,
                                                        const int32_t *__restrict__ eta_r, int64_t k0, double *__restrict__ part) {
    __shared__ double sm[4];
    const int64_t k = k0 + blockIdx.y;
    const int r = eta_r[k];
    const double *alpha = eta + static_cast<size_t>(k) * m;
    double acc = 0.0;
    for (int64_t p = static_cast<int64_t>(blockIdx.x) * TB_WG + threadIdx.x; p < m; p += static_cast<int64_t>(gridDim.x) * TB_WG)
        if (p != r) {
            const double a = alpha[p];
            if (a != 0.0) acc += a * v[p];
        }
    const double tot = tb_block_sum(acc, sm);
    if (threadIdx.x == 0) part[blockIdx.y * TB_ETS + blockIdx.x] = tot;
}
__global__ __launch_bounds__(64) void k_tb_etat_solve(int64_t m, int nslice, int K, double *__restrict__ v, const double *__restrict__ eta,
                                                      const int32_t *__restrict__ eta_r, int64_t k0, const double *__restrict__ part) {
    __shared__ double sM[TB_EB * TB_EB]; // sM[i][j] = alpha_i[r_j] (j > i, r_j != r_i): what step j's change adds to step i's dot
    __shared__ int sr[TB_EB];
    const int j = threadIdx.x;
    sr[j] = (j < K) ? eta_r[k0 + j] : -1;
    __syncthreads();
    for (int e = j; e < TB_EB * TB_EB; e += 64) {
        const int i = e / TB_EB, jj = e % TB_EB;
        double x = 0.0;
        if (i < K && jj < K && jj > i && sr[jj] != sr[i]) x = eta[static_cast<size_t>(k0 + i) * m + sr[jj]];
        sM[e] = x;
    }
    double dot = 0.0, cur = 0.0, diag = 1.0, delta = 0.0;
    if (j < K) {
        for (int g = 0; g < nslice; ++g) dot += part[j * TB_ETS + g];
        cur = v[sr[j]];
        diag = eta[static_cast<size_t>(k0 + j) * m + sr[j]];
    }
    __syncthreads();
    for (int i = K - 1; i >= 0; --i) { // lane jj holds delta of step jj (0 until it ran) and the current value at r_jj
        double t = (j > i && j < K) ? sM[i * TB_EB + j] * delta : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        const double s_i = __shfl(dot, i, 64) + t;
        const double cur_i = __shfl(cur, i, 64);
        const double nw = (cur_i - s_i) / __shfl(diag, i, 64);
        if (j == i) delta = nw - cur_i;
        if (j <= i && sr[j] == sr[i]) cur = nw; // (older etas of the block on the same position see the new value)
    }
    // the value a position ends with is that of the OLDEST eta of the block on it
    if (j < K) {
        bool last = true;
        for (int q = 0; q < j; ++q) last = last && (sr[q] != sr[j]);
        if (last) v[sr[j]] = cur;
    }
}

struct DevBufs {
    std::vector<void *> p;
    ~DevBufs() {
        for (void *q : p) (void)sx_dfree(q);
    }
    template <class T>
    int get(size_t count, T **out) {
        void *d = nullptr;
        if (sx_dmalloc(&d, sizeof(T) * (count ? count : 1)) != hipSuccess) {
            sx_set_error("hipMalloc of %zu bytes failed in the sparse crossover", sizeof(T) * count);
            return SX_ERR_NOMEM;
        }
        p.push_back(d);
        *out = static_cast<T *>(d);
        return SX_OK;
    }
};

template <class T>
int up(hipStream_t s, T *dst, const std::vector<T> &src) {
    if (!src.empty()) SX_HIP(hipMemcpyAsync(dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice, s));
    return SX_OK;
}
template <class T>
int down(hipStream_t s, std::vector<T> &dst, const T *src, size_t count) {
    dst.resize(count);
    if (count) SX_HIP(hipMemcpyAsync(dst.data(), src, sizeof(T) * count, hipMemcpyDeviceToHost, s));
    return SX_OK;
}

inline unsigned gridof(int64_t n) { return static_cast<unsigned>(n > 0 ? (n + TB_WG - 1) / TB_WG : 1); }
inline unsigned gridcap(int64_t n) { return static_cast<unsigned>(std::min<int64_t>(gridof(n), 1 << 20)); } // for grid-stride kernels


// The two big blocks of an epoch -- eta file and tableau, tens of GB at 1e6 rows -- out of ONE block that a helper thread
// allocates while the host matches columns to rows: hipMalloc of a block that size takes as long as the matching itself
// (0.5-1.4 s for the 28 GB of config-5 size, box by box; sx_internal.h: the context keeps the block between calls and a
// backend can ask for it before its first-order stage)
struct BigArena {
    sx_ctx *ctx = nullptr;
    void *base = nullptr;
    size_t bytes = 0, used = 0;
    bool started = false;
    // the context's block when it is there (a backend that asked for it ahead of the call, or the last call's), else a
    // prefetch of our own, taken when it is first needed
    void start(sx_ctx *c, size_t want) {
        ctx = c;
        started = true;
        if (sx_ctx_take_block(ctx, want - want / 3, &base, &bytes)) return; // (a block a third short of the estimate will do)
        bytes = want;
        (void)sx_ctx_prefetch_block(ctx, want);
    }
    void join() {
        if (started && !base) {
            size_t got = 0;
            if (sx_ctx_take_block(ctx, bytes - bytes / 3, &base, &got)) bytes = got;
            else bytes = 0;
            started = false;
        }
    }
    void *take(size_t n) { // nullptr: no room (the caller allocates for itself)
        join();
        n = (n + 255) & ~static_cast<size_t>(255);
        if (!base || used + n > bytes) return nullptr;
        void *q = static_cast<char *>(base) + used;
        used += n;
        return q;
    }
    void reset() { used = 0; }
    ~BigArena() {
        join();
        if (ctx && base) sx_ctx_give_block(ctx, base, bytes); // (kept for the next call of the process)
    }
};

// per-slot arrays of the tableau (one slot per tracked column) and the tableau itself; grown when pricing brings in more
// columns than there is room for.  THE list of the per-slot arrays -- (type, name, entries per slot) -- in the order they
// are allocated and freed; T, the tableau, comes before them
#define TB_SLOT_ARRAYS(X)                                                                                                          \
    X(double, xJ, 1) X(double, lJ, 1) X(double, uJ, 1) X(double, cJ, 1) X(double, dJ, 1) X(double, d1, 1) X(double, rowbuf, 1)     \
    X(double, vbuf, TB_K) X(double, ebG, TB_EB) X(double, ebS, TB_EB)                                                             \
    X(int32_t, varJ, 1) X(int32_t, statJ, 1) X(int32_t, s0, 1) X(int32_t, sbase, 1) X(int32_t, elist, 1)
struct TbSlotArrays {
    int64_t mp = 0, cap = 0;
    bool T_own = true; // false: T is a piece of the call's arena
    double *T = nullptr;
#define TB_DECLARE(type, name, per) type *name = nullptr;
    TB_SLOT_ARRAYS(TB_DECLARE)
#undef TB_DECLARE
};
struct TbSlots : TbSlotArrays {
    TbSlots() = default;
    TbSlots(const TbSlots &) = delete;
    TbSlots &operator=(const TbSlots &) = delete;
    ~TbSlots() {
        if (T_own) (void)sx_dfree(T);
#define TB_FREE(type, name, per) (void)sx_dfree(name);
        TB_SLOT_ARRAYS(TB_FREE)
#undef TB_FREE
    }
    void swap_with(TbSlots &o) { std::swap(static_cast<TbSlotArrays &>(*this), static_cast<TbSlotArrays &>(o)); }
    static size_t bytes_for(int64_t mp_, int64_t cap_) {
        return sizeof(double) * (static_cast<size_t>(mp_) * cap_ + static_cast<size_t>(7 + TB_K + 2 * TB_EB) * cap_) + sizeof(int32_t) * 5 * static_cast<size_t>(cap_);
    }
    // capacity newcap, the first `keep` slots (and tableau columns) carried over
    int reserve(hipStream_t s, int64_t mp_, int64_t newcap, int64_t keep, BigArena *arena = nullptr) {
        if (newcap <= cap && mp_ == mp) return SX_OK;
        TbSlots nw;
        nw.mp = mp_;
        nw.cap = newcap;
        const size_t c = static_cast<size_t>(newcap);
        if (arena) {
            nw.T = static_cast<double *>(arena->take(sizeof(double) * static_cast<size_t>(mp_) * c));
            nw.T_own = nw.T == nullptr;
        }
#define TB_GET(type, field, per)                                                                                                   \
    if (sx_dmalloc(reinterpret_cast<void **>(&nw.field), sizeof(type) * (static_cast<size_t>(per) * c)) != hipSuccess) {           \
        sx_set_error("hipMalloc of %zu bytes failed in the sparse crossover (tableau of %lld columns over %lld positions)",        \
                     sizeof(type) * (static_cast<size_t>(per) * c), (long long)newcap, (long long)mp_);                            \
        return SX_ERR_NOMEM;                                                                                                       \
    }
        if (!nw.T) TB_GET(double, T, mp_)
        TB_SLOT_ARRAYS(TB_GET)
#undef TB_GET
        if (keep > 0) { // (what a slot carries from round to round; the other arrays are scratch)
            SX_REQUIRE(mp_ == mp && keep <= cap, "internal: tableau columns cannot be carried over");
            const size_t k = static_cast<size_t>(keep);
            SX_HIP(hipMemcpyAsync(nw.T, T, sizeof(double) * static_cast<size_t>(mp_) * k, hipMemcpyDeviceToDevice, s));
            SX_HIP(hipMemcpyAsync(nw.xJ, xJ, sizeof(double) * k, hipMemcpyDeviceToDevice, s));
            SX_HIP(hipMemcpyAsync(nw.lJ, lJ, sizeof(double) * k, hipMemcpyDeviceToDevice, s));
            SX_HIP(hipMemcpyAsync(nw.uJ, uJ, sizeof(double) * k, hipMemcpyDeviceToDevice, s));
            SX_HIP(hipMemcpyAsync(nw.cJ, cJ, sizeof(double) * k, hipMemcpyDeviceToDevice, s));
            SX_HIP(hipMemcpyAsync(nw.dJ, dJ, sizeof(double) * k, hipMemcpyDeviceToDevice, s));
            SX_HIP(hipMemcpyAsync(nw.varJ, varJ, sizeof(int32_t) * k, hipMemcpyDeviceToDevice, s));
            SX_HIP(hipMemcpyAsync(nw.statJ, statJ, sizeof(int32_t) * k, hipMemcpyDeviceToDevice, s));
        }
        SX_HIP(hipMemsetAsync(nw.s0, 0, sizeof(int32_t) * c, s));       // no pending update anywhere
        SX_HIP(hipMemsetAsync(nw.sbase, 0xFF, sizeof(int32_t) * c, s)); // (-1: every slot's base column is T's)
        SX_HIP(hipStreamSynchronize(s));
        swap_with(nw); // (nw's destructor frees the old arrays)
        return SX_OK;
    }
};

namespace pl = sx_plan;

// ---------------------------------------------------------------------------------------------- state of a call
// host copies of the LP (once per call).  Variables: [0, n) columns of A, n + i the logical of row i ('<' rows: >= 0, others 0)
struct HostLp {
    int64_t m = 0, n = 0, nnz = 0;
    std::vector<int64_t> cptr, rptr;
    std::vector<int32_t> cidx;
    std::vector<double> cval, b, c, l, u;
    std::vector<uint8_t> lt;
    std::vector<int8_t> vb_in, cb_in;
    double lo(int64_t v) const { return v < n ? l[v] : 0.0; }
    double up(int64_t v) const { return v < n ? u[v] : (lt[v - n] ? INFINITY : 0.0); }
    double cost(int64_t v) const { return v < n ? c[v] : 0.0; }
    pl::Csc csc() const { return pl::Csc{m, n, cptr.data(), cidx.data(), cval.data()}; }
};

// what lives as long as the call: arguments, device blocks, counters, the verdict so far
struct BandCall {
    sx_ctx *ctx = nullptr;
    const sx_matrix *A = nullptr;
    const double *b = nullptr, *c = nullptr; // (device)
    hipStream_t s = nullptr;
    bool trace = false, given = false;
    double t_begin = 0.0;
    int64_t m = 0, n = 0, max_iter = 0;
    double feas_tol = 0.0, opt_tol = 0.0;
    // smallest pivot the two LUs accept.  A GUESSED basis (the m largest margins of a first-order point) may hold columns
    // that are all but dependent -- its basic solution then lies far from the point and phase 1 pays for it pivot by pivot
    // -- so its LUs set such columns aside (they stay superbasic, a logical takes their place); a basis the simplex has
    // reached, or one that was given, is kept unless it is singular to working accuracy
    double tol_band_guess = 1e-3, tol_schur_guess = 1e-1;
    static constexpr double tol_band_keep = 1e-7, tol_schur_keep = 1e-9;
    DevBufs dev; // lives as long as the call
    BigArena arena;
    double *d_tmpm = nullptr, *d_tmpn = nullptr, *d_rc = nullptr, *d_gu = nullptr, *d_ebM = nullptr;
    TbState *d_st = nullptr;
    int32_t *d_pr = nullptr;
    long long tot_iters = 0, tot_pivots = 0, tot_flips = 0, tot_degen = 0;
    int64_t added_total = 0;
    int epochs = 0, final_status = 4, bad_epochs = 0, check_epochs = 0;
    std::vector<double> hy, hslack;
    double viol_max = 0.0, resid_max = 0.0;
    size_t peak_bytes = 0;
    bool strict_next = false, strict_tried = false;
    static double now() {
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
    }
    double ms() const { return now() - t_begin; }
};

// One epoch: a factorisation of the current basic set and the simplex rounds on it.  The device side is released in the
// reverse order of the members: tableau, border operators, the two LUs, then the epoch's arrays.
struct Epoch {
    DevBufs dev;
    struct Factors {
        sx_bandlu *lu = nullptr;
        sx_denselu *dl = nullptr;
        ~Factors() {
            if (lu) sx_bandlu_destroy(lu);
            if (dl) sx_denselu_destroy(dl);
        }
    } fac;
    SxBorderOps ops;
    TbSlots sl;
    // the plan (sx_band_plan.h)
    pl::Matching mt;
    pl::EpochGeometry g;
    pl::BandTriplets tri;
    std::vector<int32_t> ph_row; // the row whose unit vector a placeholder is
    pl::Border bd;
    std::vector<int64_t> head;
    std::vector<int32_t> varJ;
    int64_t nrep = 0, nb = 0, mp = 0, nJ = 0, n_dummy = 0, EPOCH = 0;
    // device arrays over the positions
    int nblk = 0;
    int32_t *d_eqidx = nullptr, *d_eta_r = nullptr, *d_head = nullptr, *d_blist = nullptr, *d_infoff = nullptr, *d_inflist = nullptr;
    double *d_eta = nullptr, *d_xB = nullptr, *d_lB = nullptr, *d_uB = nullptr, *d_cB = nullptr, *d_g = nullptr, *d_vec = nullptr, *d_part = nullptr,
           *d_infpart = nullptr, *d_etp = nullptr;
    TbPart *d_rpart = nullptr;
    // the simplex rounds and what they leave
    TbState hst{};
    bool restart = false;
    std::vector<double> hrc; // reduced costs of the structural columns under the last duals
    std::vector<int32_t> hh, hvarJ, hstatJ;
    std::vector<double> hxb, hxJ;
};

// ---------------------------------------------------------------------------------------------- helpers
// b - A x to the host (one K2 walk), synchronised.  x on the device ...
int slack_to_host(BandCall &C, const double *d_x, std::vector<double> &out) {
    SX_TRY(sx_score_rows_dev(C.ctx, C.A, d_x, C.b, nullptr, 0.0, C.d_tmpm, nullptr));
    SX_TRY(down(C.s, out, C.d_tmpm, static_cast<size_t>(C.m)));
    SX_HIP(hipStreamSynchronize(C.s));
    return SX_OK;
}
// ... or on the host
int slack_to_host(BandCall &C, const std::vector<double> &x, std::vector<double> &out) {
    SX_TRY(up(C.s, C.d_tmpn, x));
    return slack_to_host(C, C.d_tmpn, out);
}
// vstat from the device's head / varJ: 1 basic, 2 tracked (3: tracked and superbasic, when the slots' status is given)
void vstat_from_device(const std::vector<int32_t> &hh, const std::vector<int32_t> &hvarJ, const std::vector<int32_t> *hstatJ, std::vector<int8_t> &vstat) {
    std::fill(vstat.begin(), vstat.end(), 0);
    for (int32_t v : hh)
        if (v >= 0) vstat[v] = 1;
    for (size_t t = 0; t < hvarJ.size(); ++t) vstat[hvarJ[t]] = (hstatJ && (*hstatJ)[t] == TB_SUP) ? 3 : 2;
}
// the basic variables' values -> the point; returns the largest bound violation among them
double basic_values_to_point(const HostLp &lp, const std::vector<int32_t> &hh, const std::vector<double> &hxb, std::vector<double> &hx) {
    double viol = 0.0;
    for (size_t p = 0; p < hh.size(); ++p) {
        const int64_t v = hh[p];
        if (v < 0) continue;
        viol = std::max(viol, std::max(lp.lo(v) - hxb[p], hxb[p] - lp.up(v)));
        if (v < lp.n) hx[v] = hxb[p];
    }
    return viol;
}
// largest row residual of the point whose slacks are hslack, relative to 1 + |b_i|
double row_residual(const HostLp &lp, const std::vector<double> &hslack) {
    double worst = 0.0;
    for (int64_t i = 0; i < lp.m; ++i) {
        const double sc = 1.0 + std::fabs(lp.b[i]);
        const double r = lp.lt[i] ? std::max(-hslack[i], 0.0) : std::fabs(hslack[i]);
        worst = std::max(worst, r / sc);
    }
    return worst;
}
// columns of the eta file that 16 GB, or 0.4 of the free memory, hold over mp positions (the arena's estimate and the
// epoch's real length both start from this)
double eta_columns_by_memory(size_t free_b, double mp) { return std::min(16.0e9, 0.4 * static_cast<double>(free_b)) / (8.0 * mp); }

int rows_to_dev(BandCall &C, Epoch &E, const pl::HostRows &R, int64_t nrows, bool with_list, SxRowsDev &out) {
    int64_t *dp = nullptr;
    int32_t *di = nullptr, *dlist = nullptr;
    double *dv = nullptr;
    SX_TRY(E.dev.get(R.ptr.size(), &dp));
    SX_TRY(E.dev.get(R.idx.size(), &di));
    SX_TRY(E.dev.get(R.val.size(), &dv));
    SX_TRY(up(C.s, dp, R.ptr));
    SX_TRY(up(C.s, di, R.idx));
    SX_TRY(up(C.s, dv, R.val));
    if (with_list) {
        SX_TRY(E.dev.get(R.list.size(), &dlist));
        SX_TRY(up(C.s, dlist, R.list));
    }
    out.nrows = nrows;
    out.ptr = dp;
    out.idx = di;
    out.val = dv;
    out.list = dlist;
    return SX_OK;
}

// solve helper: row-space columns through the bordered factors, then the eta file
int ftran_cols(BandCall &C, Epoch &E, double *W, int64_t ncols, int64_t n_eta_now, bool lp_columns) {
    if (ncols == 0) return SX_OK;
    hipStream_t s = C.s;
    const int64_t mp = E.mp;
    SX_TRY(E.ops.ftran(W, ncols, lp_columns));
    if (n_eta_now > 0) { // (what the tableau would drop anyway goes first: the list of an eta holds real entries only)
        hipLaunchKernelGGL(k_tb_drop, dim3(gridcap(mp * ncols)), dim3(TB_WG), 0, s, mp * ncols, W, TB_DROP);
    }
    for (int64_t k0 = 0; k0 < n_eta_now; k0 += TB_EB) {
        const int K = static_cast<int>(std::min<int64_t>(TB_EB, n_eta_now - k0));
        hipLaunchKernelGGL(k_tb_etab_gather, dim3(gridof(std::max<int64_t>(TB_EB * ncols, TB_EB * TB_EB))), dim3(TB_WG), 0, s, mp, ncols, W, E.d_eta,
                           E.d_eta_r, k0, K, E.sl.ebG, C.d_ebM);
        hipLaunchKernelGGL(k_tb_etab_solve, dim3(static_cast<unsigned>((ncols + 63) / 64)), dim3(64), 0, s, ncols, E.sl.ebG, C.d_ebM, E.sl.ebS, E.sl.elist);
        hipLaunchKernelGGL(k_tb_etab_apply, dim3(static_cast<unsigned>(std::min(E.nblk, 1024)), static_cast<unsigned>((ncols + TB_EC - 1) / TB_EC)),
                           dim3(TB_WG), 0, s, mp, ncols, W, E.d_eta, E.d_eta_r, k0, K, E.sl.ebS, E.sl.elist);
    }
    SX_HIP(hipGetLastError());
    return SX_OK;
}

// ---------------------------------------------------------------------------------------------- stages before the epochs
// The question "would the band LU take the matched basis?" has a sufficient answer in the matrix alone: no column of
// A is taller (over the rows that are not dense) than a band the LU takes, so no basis is.  One kernel instead of the
// host copies, the row order and the matching (18 ms at 1e5 rows); a matrix that fails it gets the full answer
int probe_shortcut(BandCall &C, bool &taken) {
    const sx_matrix *A = C.A;
    const int64_t dense_thr = pl::dense_threshold(A->nnz, C.m);
    int *d_q = nullptr;
    SX_TRY(C.dev.get(2, &d_q));
    SX_HIP(hipMemsetAsync(d_q, 0, 2 * sizeof(int), C.s));
    hipLaunchKernelGGL(k_tb_colspan, dim3(gridof(std::max(C.m, C.n))), dim3(TB_WG), 0, C.s, C.m, C.n, A->csc_ptr, A->csc_idx, A->csr_ptr, dense_thr, d_q);
    int hq[2] = {0, 0};
    SX_HIP(hipMemcpyAsync(hq, d_q, sizeof(hq), hipMemcpyDeviceToHost, C.s));
    SX_HIP(hipStreamSynchronize(C.s));
    if (C.trace) fprintf(stderr, "[sx_crossover_band] probe: tallest column %d rows outside the %d dense rows\n", hq[0], hq[1]);
    taken = hq[1] <= pl::MAX_NB / 2 && sx_bandlu_supports(hq[0], hq[0]);
    return SX_OK;
}

int host_copies(BandCall &C, const double *l, const double *u, const uint8_t *row_is_lt, const double *x_start, const int8_t *vbasis_in,
                const int8_t *cbasis_in, HostLp &lp, pl::BasisState &bs) {
    const sx_matrix *A = C.A;
    hipStream_t s = C.s;
    const int64_t m = C.m, n = C.n;
    lp.m = m;
    lp.n = n;
    lp.nnz = A->nnz;
    lp.lt.assign(static_cast<size_t>(m), 0);
    SX_TRY(down(s, lp.cptr, A->csc_ptr, static_cast<size_t>(n) + 1));
    SX_TRY(down(s, lp.rptr, A->csr_ptr, static_cast<size_t>(m) + 1));
    SX_TRY(down(s, lp.cidx, A->csc_idx, static_cast<size_t>(A->nnz)));
    SX_TRY(down(s, lp.cval, A->csc_val, static_cast<size_t>(A->nnz)));
    SX_TRY(down(s, lp.b, C.b, static_cast<size_t>(m)));
    SX_TRY(down(s, lp.c, C.c, static_cast<size_t>(n)));
    SX_TRY(down(s, lp.l, l, static_cast<size_t>(n)));
    SX_TRY(down(s, lp.u, u, static_cast<size_t>(n)));
    SX_TRY(down(s, bs.hx, x_start, static_cast<size_t>(n)));
    if (row_is_lt) SX_HIP(hipMemcpyAsync(lp.lt.data(), row_is_lt, static_cast<size_t>(m), hipMemcpyDeviceToHost, s));
    if (vbasis_in) {
        SX_TRY(down(s, lp.vb_in, vbasis_in, static_cast<size_t>(n)));
        SX_TRY(down(s, lp.cb_in, cbasis_in, static_cast<size_t>(m)));
    }
    SX_TRY(C.dev.get(static_cast<size_t>(m), &C.d_tmpm));
    SX_TRY(C.dev.get(static_cast<size_t>(n), &C.d_tmpn));
    SX_TRY(C.dev.get(static_cast<size_t>(n), &C.d_rc));
    SX_HIP(hipStreamSynchronize(s));
    for (int64_t j = 0; j < n; ++j) bs.hx[j] = std::min(std::max(bs.hx[j], lp.l[j]), lp.u[j]);
    return SX_OK;
}

// dense rows, band rows and the order of the band rows (once per call)
int plan_rows(BandCall &C, const HostLp &lp, pl::RowPlan &rp) {
    const sx_matrix *A = C.A;
    const int64_t dense_thr = pl::dense_threshold(A->nnz, C.m);
    pl::classify_rows(C.m, lp.rptr.data(), dense_thr, rp);
    const int64_t m1 = static_cast<int64_t>(rp.rows_band.size()), ndr = static_cast<int64_t>(rp.rows_dense.size());
    if (ndr > pl::MAX_NB) {
        sx_set_error("%lld rows with more than %lld entries: the border of the basis would pass the dense LU's %lld rows", (long long)ndr,
                     (long long)dense_thr, (long long)pl::MAX_NB);
        return SX_ERR_UNSUPPORTED;
    }
    const int32_t tall_nat = pl::tallest(lp.csc(), rp.rows_band);
    if (tall_nat > pl::CM_TRIGGER && m1 > 1) { // (the rows of A by row come to the host only when they are needed)
        std::vector<int32_t> ridx, cm;
        SX_TRY(down(C.s, ridx, A->csr_idx, static_cast<size_t>(A->nnz)));
        SX_HIP(hipStreamSynchronize(C.s));
        if (pl::cuthill_mckee_order(lp.csc(), lp.rptr.data(), ridx.data(), A->nnz, rp.rows_band, cm)) {
            const int32_t tall_cm = pl::tallest(lp.csc(), cm);
            if (C.trace) fprintf(stderr, "[sx_crossover_band] tallest column: %d rows in natural order, %d in Cuthill-McKee order\n", tall_nat, tall_cm);
            if (tall_cm < tall_nat) rp.rows_band = cm;
        }
    }
    pl::finish_row_plan(C.m, rp);
    int32_t *d_eqidx = nullptr;
    SX_TRY(C.dev.get(rp.eqidx.size(), &d_eqidx));
    SX_TRY(up(C.s, d_eqidx, rp.eqidx));
    return SX_OK;
}

int first_basic_set(BandCall &C, const HostLp &lp, const pl::RowPlan &rp, const double *x_start, pl::BasisState &bs) {
    const int64_t m = C.m, n = C.n;
    bs.init(n, m);
    if (C.given) pl::basic_set_from_codes(n, m, lp.vb_in.data(), lp.cb_in.data(), lp.l.data(), lp.u.data(), bs);
    else {
        SX_TRY(slack_to_host(C, x_start, C.hslack)); // slack = b - A x
        const size_t ncand = pl::basic_set_from_margins(n, m, lp.l.data(), lp.u.data(), lp.b.data(), lp.lt.data(), C.hslack.data(), bs);
        if (C.trace) fprintf(stderr, "[sx_crossover_band] m=%lld n=%lld: %zu interior candidates, band rows %lld, dense rows %lld\n", (long long)m, (long long)n, ncand, (long long)rp.rows_band.size(), (long long)rp.rows_dense.size());
    }
    if (C.trace) fprintf(stderr, "[sx_crossover_band] host copies, row order and first basic set at %.1f ms\n", C.ms());
    return SX_OK;
}

// the big blocks, allocated beside the matching, and the small per-call blocks
int call_blocks(BandCall &C, int64_t ndr0, size_t ntracked) {
    const int64_t m = C.m;
    size_t free_b = 0, total_b = 0;
    SX_HIP(hipMemGetInfo(&free_b, &total_b));
    // (estimates before the matching: border = dense rows + up to 32 separators of ~128 rows; a twelfth of the border is
    //  set aside by the dense LU of a guess -- 1,032 of 13,771 at config-5 size, 158 of 2,299 at the headline size)
    const double mp_est = static_cast<double>(m) + static_cast<double>(ndr0) + 33.0 * 400.0 + 2048.0;
    const double nb_est = static_cast<double>(ndr0) + 32.0 * 128.0 + 1024.0;
    const double track_est = static_cast<double>(ntracked) + nb_est / 12.0;
    const double epoch_est = std::min(std::min(20000.0, eta_columns_by_memory(free_b, mp_est)), 4.0 * (track_est + nb_est / 8.0) + 2048.0);
    const double want = 8.0 * mp_est * (epoch_est + 2.0 + 1.5 * track_est + 712.0);
    if (want > 2.0e9 && want < 0.6 * static_cast<double>(free_b) && !getenv("SX_BAND_NO_ARENA")) C.arena.start(C.ctx, static_cast<size_t>(want));
    SX_TRY(C.dev.get(1, &C.d_st));
    SX_TRY(C.dev.get(static_cast<size_t>(TB_K), &C.d_pr));
    SX_TRY(C.dev.get(static_cast<size_t>(TB_K), &C.d_gu));
    SX_TRY(C.dev.get(static_cast<size_t>(TB_EB) * TB_EB, &C.d_ebM));
    C.hy.assign(static_cast<size_t>(m), 0.0);
    return SX_OK;
}

// ---------------------------------------------------------------------------------------------- stages of an epoch
// blocks, the epoch's row maps on the device, band triplets
int epoch_geometry(BandCall &C, const HostLp &lp, const pl::RowPlan &rp, Epoch &E) {
    const int64_t m1_all = static_cast<int64_t>(rp.rows_band.size());
    const int64_t want = getenv("SX_BAND_BLOCKS") ? atoll(getenv("SX_BAND_BLOCKS")) : pl::default_block_count(m1_all);
    pl::make_geometry(lp.csc(), rp, E.mt, want, E.g);
    SX_TRY(E.dev.get(E.g.eqidx.size(), &E.d_eqidx));
    SX_TRY(up(C.s, E.d_eqidx, E.g.eqidx));
    pl::band_triplets(lp.csc(), lp.nnz, E.g, E.tri);
    if (!sx_bandlu_supports(E.tri.kl, E.tri.ku)) {
        sx_set_error("the basis is not a band matrix in the order of the rows (kl = %d, ku = %d after setting %lld dense rows aside)", E.tri.kl, E.tri.ku,
                     (long long)E.g.ndr);
        return SX_ERR_UNSUPPORTED;
    }
    if (C.trace) fprintf(stderr, "[sx_crossover_band] epoch %d: matching and band assembly done at %.1f ms\n", C.epochs, C.ms());
    return SX_OK;
}

// factor B11
int factor_band(BandCall &C, Epoch &E, bool guessed) {
    const pl::EpochGeometry &g = E.g;
    const int64_t m1 = g.m1, P = g.P;
    hipStream_t s = C.s;
    E.ph_row.assign(static_cast<size_t>(m1), -1);
    if (m1 > 0) {
        int32_t *d_trow = nullptr, *d_tcol = nullptr;
        double *d_tval = nullptr;
        DevBufs tdev;
        SX_TRY(tdev.get(E.tri.row.size(), &d_trow));
        SX_TRY(tdev.get(E.tri.col.size(), &d_tcol));
        SX_TRY(tdev.get(E.tri.val.size(), &d_tval));
        SX_TRY(up(s, d_trow, E.tri.row));
        SX_TRY(up(s, d_tcol, E.tri.col));
        SX_TRY(up(s, d_tval, E.tri.val));
        SX_TRY(sx_bandlu_create_dev(C.ctx, m1, E.tri.kl, E.tri.ku, static_cast<int64_t>(E.tri.val.size()), d_trow, d_tcol, d_tval, &E.fac.lu));
        std::vector<int32_t> rep(static_cast<size_t>(m1)), piv(static_cast<size_t>(m1));
        SX_TRY(sx_bandlu_factor_blocks_dev(E.fac.lu, guessed ? C.tol_band_guess : C.tol_band_keep, static_cast<int>(P), P > 1 ? g.stride : m1, P > 1 ? g.RL : m1,
                                            P > 1 ? g.RL_last : m1, &E.nrep, rep.data(), piv.data()));
        pl::after_band_lu(E.g, E.mt, rep, piv, E.ph_row);
    }
    if (C.trace) fprintf(stderr, "[sx_crossover_band] epoch %d: band LU done at %.1f ms (kl=%d ku=%d, %lld blocks of %lld positions with separators of %lld, %lld columns set aside)\n", C.epochs, C.ms(), E.tri.kl, E.tri.ku, (long long)P, (long long)g.RL, (long long)g.Wsep, (long long)E.nrep);
    return SX_OK;
}

// the border: as many columns as rows; then the eta file and B21
int make_border(BandCall &C, const HostLp &lp, pl::BasisState &bs, Epoch &E, bool guessed) {
    if (!pl::balance_border(C.n, E.g, E.mt, E.ph_row, guessed, bs, E.bd)) {
        sx_set_error("the border of the basis has %lld rows and %zu columns (at most %lld rows)", (long long)(E.g.ndr + E.bd.h), E.bd.bcol.size(), (long long)pl::MAX_NB);
        return SX_ERR_UNSUPPORTED;
    }
    const int64_t m1 = E.g.m1, nb = E.bd.nb(E.g), mp = m1 + nb;
    E.nb = nb;
    E.mp = mp;
    // the eta file of this epoch -- allocated now because its memory doubles as the work block of the Schur complement's
    // assembly (a block of 24 GB allocated and freed for that alone cost 0.3 s at 1e5 rows and 1.2 s at 1e6: hipFree of a
    // touched block).  Basis changes before the basis is factored afresh: a few times the columns that can move, within
    // 16 GB; a fresh factorisation keeps every basic variable (bordered form), so the file need not be long
    size_t free_b = 0, total_b = 0;
    SX_HIP(hipMemGetInfo(&free_b, &total_b));
    const int64_t by_memory = std::max<int64_t>(64, static_cast<int64_t>(eta_columns_by_memory(free_b, static_cast<double>(mp))) - 1);
    E.EPOCH = std::min<int64_t>(std::min<int64_t>(20000, by_memory), 4 * static_cast<int64_t>(bs.tracked.size() + static_cast<size_t>(nb) / 8) + 2048);
    if (const char *e = getenv("SX_BAND_EPOCH")) E.EPOCH = std::max<int64_t>(16, atoll(e));
    C.arena.reset(); // (what the last epoch held there is dead)
    E.d_eta = static_cast<double *>(C.arena.take(sizeof(double) * static_cast<size_t>(mp) * (E.EPOCH + 1)));
    if (!E.d_eta) SX_TRY(E.dev.get(static_cast<size_t>(mp) * (E.EPOCH + 1), &E.d_eta));
    SX_TRY(E.dev.get(static_cast<size_t>(E.EPOCH) + 2, &E.d_eta_r));
    // ---- B21: the dense rows' entries in the band columns, one unit entry per placeholder row
    SxBorderOps &ops = E.ops;
    ops.ctx = C.ctx;
    ops.m1 = m1;
    ops.nb = nb;
    ops.mp = mp;
    ops.lu = E.fac.lu;
    ops.tiny = TB_TINY;
    if (nb > 0) {
        pl::HostRows b21r, b21c;
        pl::b21_blocks(lp.csc(), E.g, E.bd, b21r, b21c);
        SX_TRY(rows_to_dev(C, E, b21r, nb, false, ops.b21_rows));
        SX_TRY(rows_to_dev(C, E, b21c, static_cast<int64_t>(b21c.list.size()), true, ops.b21_cols));
    }
    return SX_OK;
}

// the Schur complement, a block of border columns at a time: S[:, j] = (a2 - B21 B11^-1 a1) of column j
int schur_complement(BandCall &C, pl::BasisState &bs, Epoch &E, bool guessed) {
    const sx_matrix *A = C.A;
    hipStream_t s = C.s;
    SxBorderOps &ops = E.ops;
    const int64_t nb = E.nb, mp = E.mp, m1 = E.g.m1, EPOCH = E.EPOCH;
    int64_t nrep2 = 0;
    if (nb > 0) {
        {
            size_t free_b = 0, total_b = 0;
            SX_HIP(hipMemGetInfo(&free_b, &total_b));
            ops.v_limit = static_cast<size_t>(std::min(4.0e9, 0.05 * static_cast<double>(free_b)) / 8.0);
            if (getenv("SX_BAND_NO_V")) ops.v_failed = 1;
        }
        SX_TRY(sx_denselu_create_dev(C.ctx, nb, &E.fac.dl));
        double *Sa = nullptr;
        int64_t Sld = 0;
        SX_TRY(sx_denselu_matrix(E.fac.dl, &Sa, &Sld));
        // blocks of up to 4,096 columns (in the memory of the still empty eta file: a sparse band solve is a chain of panel steps per
        // group of 8 columns whatever the number of groups, 250 columns a launch kept 31 of 256 CUs busy), taken in the
        // order of the VARIABLES -- neighbours in that order live in neighbouring rows, so the 8 columns of a group share
        // their panels -- and written to the column of S the border's own order gives them
        const int64_t CH = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nb, 4096), EPOCH + 1));
        DevBufs sdev;
        double *Wc = E.d_eta; // (the eta file is empty until the simplex starts)
        int32_t *d_bvars = nullptr, *d_dest = nullptr;
        SX_TRY(sdev.get(static_cast<size_t>(nb), &d_bvars));
        SX_TRY(sdev.get(static_cast<size_t>(nb), &d_dest));
        const std::vector<int64_t> &bcol = E.bd.bcol;
        std::vector<int32_t> order(static_cast<size_t>(nb)), bv32(static_cast<size_t>(nb));
        std::iota(order.begin(), order.end(), 0);
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t bb) { return bcol[a] < bcol[bb]; });
        for (int64_t t = 0; t < nb; ++t) bv32[t] = static_cast<int32_t>(bcol[order[t]]);
        SX_TRY(up(s, d_bvars, bv32));
        SX_TRY(up(s, d_dest, order));
        C.peak_bytes = std::max(C.peak_bytes, sizeof(double) * (static_cast<size_t>(mp) * (EPOCH + 1) + static_cast<size_t>(Sld) * nb));
        for (int64_t c0 = 0; c0 < nb; c0 += CH) {
            const int64_t kc = std::min<int64_t>(CH, nb - c0);
            SX_HIP(hipMemsetAsync(Wc, 0, sizeof(double) * static_cast<size_t>(mp) * kc, s));
            hipLaunchKernelGGL(k_tb_scatter_cols, dim3(gridof(kc)), dim3(TB_WG), 0, s, kc, d_bvars + c0, C.n, A->csc_ptr, A->csc_idx, A->csc_val, E.d_eqidx, Wc, mp);
            SX_TRY(ops.ftran(Wc, kc, true, true));
            SX_TRY(ops.pack_v(Wc, kc, order.data() + c0)); // (the band parts B11^-1 B12 of these columns, by their windows)
            hipLaunchKernelGGL(k_tb_copy_cols, dim3(static_cast<unsigned>(std::min<int64_t>(gridof(nb), 64)), static_cast<unsigned>(kc)), dim3(TB_WG), 0, s, nb, Wc + m1, mp,
                               d_dest + c0, Sa, Sld);
        }
        SX_HIP(hipStreamSynchronize(s));
        if (C.trace) fprintf(stderr, "[sx_crossover_band] epoch %d: Schur complement (%lld rows: %lld dense, %lld placeholders) assembled at %.1f ms\n", C.epochs, (long long)nb, (long long)E.g.ndr, (long long)E.bd.h, C.ms());
        std::vector<int32_t> rep2(static_cast<size_t>(nb)), perm2(static_cast<size_t>(nb));
        SX_TRY(sx_denselu_factor_dev(E.fac.dl, guessed ? C.tol_schur_guess : C.tol_schur_keep, &nrep2, rep2.data(), perm2.data()));
        const int64_t twice = pl::after_dense_lu(C.n, E.g, E.ph_row, rep2, perm2, bs, E.bd);
        if (twice >= 0) {
            sx_set_error("internal: the repair of the Schur complement wants logical %lld twice", (long long)twice);
            return SX_ERR_UNSUPPORTED;
        }
        SX_TRY(ops.finish_v(rep2)); // (a column that left the basis: its V column is zero, like the unit vector's that replaced it)
        if (C.trace) {
            std::vector<double> dg(static_cast<size_t>(nb));
            SX_HIP(hipMemcpy2D(dg.data(), sizeof(double), Sa, sizeof(double) * (Sld + 1), sizeof(double), static_cast<size_t>(nb), hipMemcpyDeviceToHost));
            double mn = INFINITY;
            int64_t c2 = 0, c4 = 0, c6 = 0;
            for (double d : dg) {
                const double a = std::fabs(d);
                mn = std::min(mn, a);
                c2 += a < 1e-2;
                c4 += a < 1e-4;
                c6 += a < 1e-6;
            }
            fprintf(stderr, "[sx_crossover_band] epoch %d: Schur complement factored at %.1f ms (%lld columns set aside; smallest pivot %.2e, %lld / %lld / %lld below 1e-2 / 1e-4 / 1e-6); "
                            "B11^-1 B12 %s: %.1f rows per border column, %.3f GB\n",
                    C.epochs, C.ms(), (long long)nrep2, mn, (long long)c2, (long long)c4, (long long)c6, ops.v_ready ? "packed by windows" : "not kept (solve form)",
                    static_cast<double>(ops.v_used) / static_cast<double>(nb), static_cast<double>(ops.v_used) * 8e-9);
        }
    }
    ops.dl = E.fac.dl;
    return SX_OK;
}

// B12: the border columns' entries in the band rows
int border_blocks(BandCall &C, const HostLp &lp, Epoch &E) {
    SxBorderOps &ops = E.ops;
    const int64_t nb = E.nb, m1 = E.g.m1;
    if (nb > 0 && m1 > 0) {
        pl::HostRows b12r, b12c;
        pl::b12_blocks(lp.csc(), E.g, E.bd, b12r, b12c);
        SX_TRY(rows_to_dev(C, E, b12r, static_cast<int64_t>(b12r.list.size()), true, ops.b12_rows));
        SX_TRY(rows_to_dev(C, E, b12c, nb, false, ops.b12_cols));
        ops.work_cols = ops.v_ready ? 1 : std::max<int64_t>(1, std::min<int64_t>(128, static_cast<int64_t>(1.0e9 / (8.0 * static_cast<double>(m1)))));
        SX_TRY(E.dev.get(static_cast<size_t>(m1) * ops.work_cols, &ops.work));
    }
    if (C.trace) {
        SX_HIP(hipStreamSynchronize(C.s));
        fprintf(stderr, "[sx_crossover_band] epoch %d: border blocks in place at %.1f ms\n", C.epochs, C.ms());
    }
    return SX_OK;
}

// who is where, then this epoch's blocks: positions, tableau
int epoch_arrays(BandCall &C, pl::BasisState &bs, Epoch &E) {
    int64_t bad = 0;
    const int who = pl::who_is_where(C.m, E.g, E.bd, bs, E.head, E.varJ, E.n_dummy, bad);
    if (who == 1) {
        sx_set_error("internal: variable %lld covers two positions of the basis", (long long)bad);
        return SX_ERR_UNSUPPORTED;
    }
    if (who == 2) {
        sx_set_error("internal: %lld basic variables for %lld rows", (long long)bad, (long long)C.m);
        return SX_ERR_UNSUPPORTED;
    }
    E.nJ = static_cast<int64_t>(E.varJ.size());
    const int64_t mp = E.mp, nJ = E.nJ;
    E.nblk = static_cast<int>(gridof(mp));
    const int nblk = E.nblk;
    SX_TRY(E.dev.get(static_cast<size_t>(mp), &E.d_xB));
    SX_TRY(E.dev.get(static_cast<size_t>(mp), &E.d_lB));
    SX_TRY(E.dev.get(static_cast<size_t>(mp), &E.d_uB));
    SX_TRY(E.dev.get(static_cast<size_t>(mp), &E.d_cB));
    SX_TRY(E.dev.get(static_cast<size_t>(mp), &E.d_g));
    SX_TRY(E.dev.get(static_cast<size_t>(mp), &E.d_vec));
    SX_TRY(E.dev.get(static_cast<size_t>(mp), &E.d_head));
    SX_TRY(E.dev.get(static_cast<size_t>(2 * nblk), &E.d_part));
    SX_TRY(E.dev.get(static_cast<size_t>(TB_EB) * TB_ETS, &E.d_etp));
    SX_TRY(E.dev.get(static_cast<size_t>(nblk), &E.d_blist));
    SX_TRY(E.dev.get(static_cast<size_t>(2 * nblk), &E.d_infpart));
    SX_TRY(E.dev.get(static_cast<size_t>(nblk), &E.d_infoff));
    SX_TRY(E.dev.get(static_cast<size_t>(TB_INFLIST), &E.d_inflist));
    SX_TRY(E.dev.get(static_cast<size_t>(nblk), &E.d_rpart));
    size_t free_b = 0, total_b = 0;
    SX_HIP(hipMemGetInfo(&free_b, &total_b));
    int64_t cap0 = nJ + std::max<int64_t>(512, nJ / 2); // (growing it later is an allocation, a copy and a free of GBs)
    if (static_cast<double>(TbSlots::bytes_for(mp, cap0)) > 0.6 * static_cast<double>(free_b)) cap0 = nJ + 16;
    if (static_cast<double>(TbSlots::bytes_for(mp, cap0)) > 0.8 * static_cast<double>(free_b)) {
        sx_set_error("the tableau of %lld tracked columns over %lld positions does not fit the free device memory", (long long)cap0, (long long)mp);
        return SX_ERR_NOMEM;
    }
    SX_TRY(E.sl.reserve(C.s, mp, cap0, 0, &C.arena));
    C.peak_bytes = std::max(C.peak_bytes, TbSlots::bytes_for(mp, cap0) + sizeof(double) * static_cast<size_t>(mp) * (E.EPOCH + 1));
    if (C.trace) fprintf(stderr, "[sx_crossover_band] epoch %d: tableau and position blocks allocated at %.1f ms\n", C.epochs, C.ms());
    return SX_OK;
}

// values: non-basic and tracked columns, right-hand side; the basic variables' arrays and their values x_B = B^-1 rhs
int values_and_rhs(BandCall &C, const HostLp &lp, pl::BasisState &bs, Epoch &E) {
    hipStream_t s = C.s;
    const int64_t m = C.m, n = C.n, mp = E.mp;
    std::vector<double> &hx = bs.hx;
    // logical of row i: s_i = b_i - (A x)_i for the tracked ones (their current value), 0 for the non-basic ones
    SX_TRY(slack_to_host(C, hx, C.hslack));
    std::vector<double> xN(hx);
    for (int64_t j = 0; j < n; ++j) {
        if (bs.vstat[j] == 1) xN[j] = 0.0;
        else if (bs.vstat[j] == 0) {
            const bool upb = (lp.u[j] - hx[j]) < (hx[j] - lp.l[j]);
            double v = upb ? lp.u[j] : lp.l[j];
            if (std::isinf(v)) v = 0.0;
            xN[j] = v;
            hx[j] = v;
            bs.atup[j] = upb;
        }
    }
    for (int64_t i = 0; i < m; ++i) {
        bs.xlog[i] = 0.0;
        if (bs.vstat[n + i] == 2) bs.xlog[i] = lp.lt[i] ? std::max(C.hslack[i], 0.0) : 0.0;
    }
    std::vector<double> hr;
    SX_TRY(slack_to_host(C, xN, hr));
    std::vector<double> rp(static_cast<size_t>(mp), 0.0); // (a placeholder's border row: 0)
    for (int64_t i = 0; i < m; ++i) rp[E.g.eqidx[i]] = hr[i] - bs.xlog[i];
    // ---- basic variables (a dummy -- placeholder or mirror column -- is free, costs nothing and never leaves)
    {
        std::vector<double> hlB(static_cast<size_t>(mp)), huB(static_cast<size_t>(mp)), hcB(static_cast<size_t>(mp));
        std::vector<int32_t> hhead(static_cast<size_t>(mp));
        for (int64_t p = 0; p < mp; ++p) {
            hhead[p] = static_cast<int32_t>(E.head[p]);
            if (E.head[p] < 0) {
                hlB[p] = -INFINITY;
                huB[p] = INFINITY;
                hcB[p] = 0.0;
                continue;
            }
            hlB[p] = lp.lo(E.head[p]);
            huB[p] = lp.up(E.head[p]);
            hcB[p] = lp.cost(E.head[p]);
        }
        SX_TRY(up(s, E.d_head, hhead));
        SX_TRY(up(s, E.d_lB, hlB));
        SX_TRY(up(s, E.d_uB, huB));
        SX_TRY(up(s, E.d_cB, hcB));
        SX_TRY(up(s, E.d_xB, rp));
        SX_HIP(hipStreamSynchronize(s));
    }
    if (C.trace) fprintf(stderr, "[sx_crossover_band] epoch %d: right-hand side and basic variables' arrays at %.1f ms\n", C.epochs, C.ms());
    SX_TRY(ftran_cols(C, E, E.d_xB, 1, 0, false));
    return SX_OK;
}

// A GIVEN basis is kept as it is (tolerances of a basis the simplex has reached) -- unless its basic solution says it
// is no basis to start from: members that are all but dependent put it far outside the bounds, and phase 1 would
// pay for each of them pivot by pivot (15 wrong members of 1,200: 6,537 iterations against 402 from the point alone).
// Then the same set is factored once more with the tolerances of a guess
int given_basis_is_far(BandCall &C, const HostLp &lp, Epoch &E, bool &far) {
    std::vector<double> t;
    SX_TRY(down(C.s, t, E.d_xB, static_cast<size_t>(E.mp)));
    SX_HIP(hipStreamSynchronize(C.s));
    double worst = 0.0;
    int64_t ninf = 0;
    for (int64_t p = 0; p < E.mp; ++p) {
        if (E.head[p] < 0) continue;
        const double vi = std::max(lp.lo(E.head[p]) - t[p], t[p] - lp.up(E.head[p]));
        if (vi > C.feas_tol) ++ninf;
        worst = std::max(worst, vi);
    }
    far = worst > 1.0 || ninf > std::max<int64_t>(16, C.m / 50);
    if (far && C.trace) fprintf(stderr, "[sx_crossover_band] the given basis puts %lld variables outside their bounds (worst %.3e): factored again with the tolerances of a guess\n", (long long)ninf, worst);
    return SX_OK;
}

// (trace) how far the basic solution is from the point handed over (conditioning of the guessed basis)
int trace_basic_solution(BandCall &C, const HostLp &lp, const pl::BasisState &bs, Epoch &E) {
    const int64_t n = C.n, nb = E.nb, m1 = E.g.m1;
    std::vector<double> t;
    SX_TRY(down(C.s, t, E.d_xB, static_cast<size_t>(E.mp)));
    SX_HIP(hipStreamSynchronize(C.s));
    double devi = 0.0, worst = 0.0, dummy = 0.0;
    int64_t ninf = 0, inf_bs = 0, inf_bl = 0, inf_border = 0, border_struct = 0;
    for (int64_t j = 0; j < nb; ++j) border_struct += E.bd.bcol[j] >= 0 && E.bd.bcol[j] < n;
    for (int64_t p = 0; p < E.mp; ++p) {
        const int64_t v = E.head[p];
        if (v < 0) {
            if (p < m1) dummy = std::max(dummy, std::fabs(t[p]));
            continue;
        }
        const double ref = v < n ? bs.hx[v] : (lp.lt[v - n] ? std::max(C.hslack[v - n], 0.0) : 0.0);
        devi = std::max(devi, std::fabs(t[p] - ref));
        const double vi = std::max(lp.lo(v) - t[p], t[p] - lp.up(v));
        if (vi > C.feas_tol) {
            ++ninf;
            if (p >= m1) ++inf_border;
            else if (v < n) ++inf_bs;
            else ++inf_bl;
        }
        worst = std::max(worst, vi);
    }
    fprintf(stderr, "[sx_crossover_band] epoch %d: outside their bounds: %lld band columns, %lld band logicals, %lld border variables (the border holds %lld columns, %lld logicals)\n",
            C.epochs, (long long)inf_bs, (long long)inf_bl, (long long)inf_border, (long long)border_struct, (long long)(nb - border_struct));
    fprintf(stderr, "[sx_crossover_band] epoch %d: basic solution deviates from the point by at most %.3e; %lld basic variables outside their bounds (worst %.3e); "
                    "placeholders hold at most %.1e; %.1f ms\n", C.epochs, devi, (long long)ninf, worst, dummy, C.ms());
    return SX_OK;
}

// ---- tracked columns: their slots ...
int load_slots(BandCall &C, const HostLp &lp, const pl::BasisState &bs, Epoch &E, int64_t s0, const std::vector<int32_t> &vars) {
    hipStream_t s = C.s;
    TbSlots &sl = E.sl;
    const size_t k = vars.size();
    if (k == 0) return SX_OK;
    std::vector<double> vx(k), vl(k), vu(k), vc(k);
    std::vector<int32_t> vs(k);
    for (size_t t = 0; t < k; ++t) {
        const int64_t v = vars[t];
        vl[t] = lp.lo(v);
        vu[t] = lp.up(v);
        vc[t] = lp.cost(v);
        vx[t] = std::min(std::max(v < C.n ? bs.hx[v] : bs.xlog[v - C.n], vl[t]), vu[t]);
        if (vx[t] > vl[t] && vx[t] < vu[t]) vs[t] = TB_SUP;
        else vs[t] = (vx[t] >= vu[t] && vu[t] > vl[t]) ? TB_UPP : TB_LOW;
    }
    SX_HIP(hipMemcpyAsync(sl.varJ + s0, vars.data(), sizeof(int32_t) * k, hipMemcpyHostToDevice, s));
    SX_HIP(hipMemcpyAsync(sl.xJ + s0, vx.data(), sizeof(double) * k, hipMemcpyHostToDevice, s));
    SX_HIP(hipMemcpyAsync(sl.lJ + s0, vl.data(), sizeof(double) * k, hipMemcpyHostToDevice, s));
    SX_HIP(hipMemcpyAsync(sl.uJ + s0, vu.data(), sizeof(double) * k, hipMemcpyHostToDevice, s));
    SX_HIP(hipMemcpyAsync(sl.cJ + s0, vc.data(), sizeof(double) * k, hipMemcpyHostToDevice, s));
    SX_HIP(hipMemcpyAsync(sl.statJ + s0, vs.data(), sizeof(int32_t) * k, hipMemcpyHostToDevice, s));
    SX_HIP(hipStreamSynchronize(s)); // (the staging vectors go out of scope)
    return SX_OK;
}
// ... and their tableau columns T[:, s0 .. s0 + k) = B^-1 a_j with their reduced costs
int build_cols(BandCall &C, Epoch &E, int64_t s0, int64_t k, int64_t n_eta_now) {
    if (k == 0) return SX_OK;
    const sx_matrix *A = C.A;
    hipStream_t s = C.s;
    TbSlots &sl = E.sl;
    const int64_t mp = E.mp;
    double *W = sl.T + static_cast<size_t>(s0) * mp;
    SX_HIP(hipMemsetAsync(W, 0, sizeof(double) * static_cast<size_t>(mp) * k, s));
    hipLaunchKernelGGL(k_tb_scatter_cols, dim3(gridof(k)), dim3(TB_WG), 0, s, k, sl.varJ + s0, C.n, A->csc_ptr, A->csc_idx, A->csc_val, E.d_eqidx, W, mp);
    SX_TRY(ftran_cols(C, E, W, k, n_eta_now, true));
    hipLaunchKernelGGL(k_tb_drop, dim3(gridcap(mp * k)), dim3(TB_WG), 0, s, mp * k, W, 10.0 * TB_DROP);
    // reduced costs of the new columns under the current basis: d = c_J - c_B^T T
    hipLaunchKernelGGL(k_tb_coldot, dim3(static_cast<unsigned>(k)), dim3(TB_WG), 0, s, mp, W, E.d_cB, sl.cJ + s0, sl.dJ + s0);
    SX_HIP(hipGetLastError());
    return SX_OK;
}

// the first tableau columns of the epoch and the state the device starts from
int tableau_columns(BandCall &C, const HostLp &lp, const pl::BasisState &bs, Epoch &E) {
    hipStream_t s = C.s;
    SX_TRY(load_slots(C, lp, bs, E, 0, E.varJ));
    SX_TRY(build_cols(C, E, 0, E.nJ, 0));
    if (C.trace) {
        SX_HIP(hipStreamSynchronize(s));
        fprintf(stderr, "[sx_crossover_band] epoch %d: tableau columns (FTRAN of %lld) done at %.1f ms\n", C.epochs, (long long)E.nJ, C.ms());
    }
    E.hst = TbState{};
    E.hst.max_iter = C.max_iter - C.tot_iters;
    E.hst.cap_eta = E.EPOCH;
    E.hst.feas_tol = C.feas_tol;
    E.hst.opt_tol = C.opt_tol;
    SX_HIP(hipMemcpyAsync(C.d_st, &E.hst, sizeof(E.hst), hipMemcpyHostToDevice, s));
    SX_HIP(hipStreamSynchronize(s));
    if (C.trace)
        fprintf(stderr, "[sx_crossover_band] epoch %d: %lld positions (%lld band + %lld border, %lld dummies), %lld tracked columns (tableau capacity %lld = %.2f GB, "
                        "eta file %lld = %.2f GB); %.1f ms so far\n", C.epochs, (long long)E.mp, (long long)E.g.m1, (long long)E.nb, (long long)E.n_dummy, (long long)E.nJ,
                (long long)E.sl.cap, static_cast<double>(E.mp) * E.sl.cap * 8e-9, (long long)E.EPOCH, static_cast<double>(E.mp) * (E.EPOCH + 1) * 8e-9, C.ms());
    return SX_OK;
}

// ---------------------------------------------------------------------------------------------- the simplex on the tracked columns
void one_pivot(BandCall &C, Epoch &E) {
    hipStream_t s = C.s;
    TbSlots &sl = E.sl;
    TbState *d_st = C.d_st;
    const int64_t mp = E.mp, nJ = E.nJ;
    const int nblk = E.nblk;
    const TbPend pend{sl.vbuf, C.d_pr, sl.s0, sl.sbase, sl.cap};
    hipLaunchKernelGGL(k_tb_infeas, dim3(nblk), dim3(TB_WG), 0, s, mp, E.d_xB, E.d_lB, E.d_uB, d_st, E.d_g, E.d_infpart);
    hipLaunchKernelGGL(k_tb_phase, dim3(1), dim3(TB_WG), 0, s, nblk, E.d_infpart, d_st, E.d_infoff);
    hipLaunchKernelGGL(k_tb_inflist, dim3(nblk), dim3(TB_WG), 0, s, mp, E.d_g, E.d_infpart, E.d_infoff, d_st, E.d_inflist);
    hipLaunchKernelGGL(k_tb_gu, dim3(TB_K), dim3(TB_WG), 0, s, mp, nblk, E.d_eta, E.d_g, E.d_inflist, d_st, pend, C.d_gu);
    hipLaunchKernelGGL(k_tb_price1, dim3(static_cast<unsigned>(nJ)), dim3(TB_WG), 0, s, mp, nblk, sl.T, E.d_g, E.d_inflist, d_st, pend, C.d_gu, sl.d1);
    hipLaunchKernelGGL(k_tb_select, dim3(1), dim3(TB_WG), 0, s, nJ, sl.dJ, sl.d1, sl.statJ, sl.xJ, sl.lJ, sl.uJ, d_st);
    hipLaunchKernelGGL(k_tb_ratio1, dim3(nblk), dim3(TB_WG), 0, s, mp, sl.T, E.d_xB, E.d_lB, E.d_uB, d_st, E.d_eta, E.d_part, pend);
    hipLaunchKernelGGL(k_tb_tmax, dim3(1), dim3(TB_WG), 0, s, nblk, E.d_part, d_st, E.d_blist);
    hipLaunchKernelGGL(k_tb_ratio, dim3(nblk), dim3(TB_WG), 0, s, mp, E.d_xB, E.d_lB, E.d_uB, d_st, E.d_eta, E.d_rpart);
    hipLaunchKernelGGL(k_tb_decide, dim3(1), dim3(TB_WG), 0, s, nblk, E.d_rpart, sl.xJ, sl.lJ, sl.uJ, sl.statJ, d_st);
    hipLaunchKernelGGL(k_tb_rowcopy, dim3(gridof(nJ)), dim3(TB_WG), 0, s, mp, nJ, sl.T, E.d_eta, d_st, pend, sl.rowbuf);
    hipLaunchKernelGGL(k_tb_update, dim3(static_cast<unsigned>(std::min(nblk, 64))), dim3(TB_WG), 0, s, mp, E.d_xB, E.d_eta, d_st, E.d_blist);
    hipLaunchKernelGGL(k_tb_post, dim3(1), dim3(TB_WG), 0, s, nJ, sl.dJ, sl.rowbuf, E.d_head, E.d_xB, E.d_lB, E.d_uB, E.d_cB, sl.varJ, sl.xJ, sl.lJ, sl.uJ,
                       sl.cJ, sl.statJ, E.d_eta_r, d_st, sl.vbuf, sl.cap, C.d_pr, sl.s0, sl.sbase);
}
void fold(BandCall &C, Epoch &E) { // applies the pending batch when it is nearly full, or when the run has stopped
    hipStream_t s = C.s;
    TbSlots &sl = E.sl;
    const int64_t mp = E.mp, nJ = E.nJ;
    const TbPend pend{sl.vbuf, C.d_pr, sl.s0, sl.sbase, sl.cap};
    hipLaunchKernelGGL(k_tb_fold_begin, dim3(1), dim3(1), 0, s, C.d_st, 16);
    hipLaunchKernelGGL(k_tb_fold, dim3(static_cast<unsigned>(std::min(E.nblk, 128)), static_cast<unsigned>((nJ + TB_FJ - 1) / TB_FJ)), dim3(TB_WG), 0, s,
                       mp, nJ, sl.T, E.d_eta, C.d_st, pend);
    hipLaunchKernelGGL(k_tb_fold_end, dim3(gridof(nJ)), dim3(TB_WG), 0, s, nJ, C.d_st, sl.s0, sl.sbase);
    hipLaunchKernelGGL(k_tb_fold_done, dim3(1), dim3(1), 0, s, C.d_st);
}
// pivots in batches of 16 until the device stops: E.hst.status != 0
int run_pivots(BandCall &C, Epoch &E) {
    hipStream_t s = C.s;
    TbState &hst = E.hst;
    if (E.nJ > 0) {
        for (;;) {
            for (int k = 0; k < 16; ++k) one_pivot(C, E);
            fold(C, E);
            SX_HIP(hipMemcpyAsync(&hst, C.d_st, sizeof(hst), hipMemcpyDeviceToHost, s));
            SX_HIP(hipStreamSynchronize(s));
            SX_HIP(hipGetLastError());
            if (hst.status != 0) break;
        }
    } else { // nothing tracked: only the state of the basic variables decides the phase
        hipLaunchKernelGGL(k_tb_infeas, dim3(E.nblk), dim3(TB_WG), 0, s, E.mp, E.d_xB, E.d_lB, E.d_uB, C.d_st, E.d_g, E.d_infpart);
        hipLaunchKernelGGL(k_tb_phase, dim3(1), dim3(TB_WG), 0, s, E.nblk, E.d_infpart, C.d_st, E.d_infoff);
        SX_HIP(hipMemcpyAsync(&hst, C.d_st, sizeof(hst), hipMemcpyDeviceToHost, s));
        SX_HIP(hipStreamSynchronize(s));
        hst.status = 1;
    }
    return SX_OK;
}
// no tracked column prices out: duals, then the reduced costs of every other column (E.hrc) and who is where now
// (bs.vstat).  In phase 1 the cost is the infeasibility's (g on the basic variables, nothing elsewhere)
int price_all(BandCall &C, pl::BasisState &bs, Epoch &E, int rounds, bool ph1) {
    hipStream_t s = C.s;
    const int64_t m = C.m, n = C.n, mp = E.mp;
    const TbState &hst = E.hst;
    SX_HIP(hipMemcpyAsync(E.d_vec, ph1 ? E.d_g : E.d_cB, sizeof(double) * static_cast<size_t>(mp), hipMemcpyDeviceToDevice, s));
    const int ets = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(TB_ETS, mp / 8192)));
    for (int64_t hi = hst.n_eta; hi > 0; hi -= TB_EB) { // blocks of TB_EB etas, the youngest first
        const int64_t k0 = std::max<int64_t>(0, hi - TB_EB);
        const int K = static_cast<int>(hi - k0);
        hipLaunchKernelGGL(k_tb_etat_dots, dim3(static_cast<unsigned>(ets), static_cast<unsigned>(K)), dim3(TB_WG), 0, s, mp, E.d_vec, E.d_eta, E.d_eta_r, k0, E.d_etp);
        hipLaunchKernelGGL(k_tb_etat_solve, dim3(1), dim3(64), 0, s, mp, ets, K, E.d_vec, E.d_eta, E.d_eta_r, k0, E.d_etp);
    }
    SX_TRY(E.ops.btran(E.d_vec)); // B_aug^T y = v: position space in, row space out
    std::vector<double> yeq;
    SX_TRY(down(s, yeq, E.d_vec, static_cast<size_t>(mp)));
    SX_HIP(hipStreamSynchronize(s));
    if (C.trace) fprintf(stderr, "[sx_crossover_band]   round %d: duals (eta file of %lld, transposed solves) by %.1f ms\n", rounds, (long long)hst.n_eta, C.ms());
    for (int64_t i = 0; i < m; ++i) C.hy[i] = yeq[E.g.eqidx[i]];
    // reduced costs of all structural columns with these duals (the K1 walk): rc = c' - A^T y
    SX_HIP(hipMemcpyAsync(C.d_tmpm, C.hy.data(), sizeof(double) * static_cast<size_t>(m), hipMemcpyHostToDevice, s));
    const double *cost = C.c;
    if (ph1) {
        SX_HIP(hipMemsetAsync(C.d_tmpn, 0, sizeof(double) * static_cast<size_t>(n), s));
        cost = C.d_tmpn;
    }
    SX_TRY(sx_score_columns_dev(C.ctx, C.A, C.d_tmpm, cost, nullptr, nullptr, nullptr, 0.0, C.d_rc, nullptr));
    SX_TRY(down(s, E.hrc, C.d_rc, static_cast<size_t>(n)));
    // who is where now
    std::vector<int32_t> hh, hvarJ, hstatJ;
    SX_TRY(down(s, hh, E.d_head, static_cast<size_t>(mp)));
    SX_TRY(down(s, hvarJ, E.sl.varJ, static_cast<size_t>(E.nJ)));
    SX_TRY(down(s, hstatJ, E.sl.statJ, static_cast<size_t>(E.nJ)));
    SX_HIP(hipStreamSynchronize(s));
    if (C.trace) fprintf(stderr, "[sx_crossover_band]   round %d: reduced costs by %.1f ms\n", rounds, C.ms());
    vstat_from_device(hh, hvarJ, nullptr, bs.vstat);
    return SX_OK;
}
// the columns outside the tableau that price out under E.hrc / C.hy, the worst first (ties by variable)
void violators(const BandCall &C, const HostLp &lp, const pl::BasisState &bs, const Epoch &E, std::vector<std::pair<double, int32_t>> &viol) {
    const int64_t m = C.m, n = C.n;
    const double opt_tol = C.opt_tol;
    viol.clear();
    for (int64_t j = 0; j < n; ++j) {
        if (bs.vstat[j] != 0 || lp.l[j] == lp.u[j]) continue;
        const double d = E.hrc[j];
        // a free column rests at 0 and may move either way (it loads as TB_SUP): both signs price
        const bool free_col = std::isinf(lp.l[j]) && std::isinf(lp.u[j]);
        if (free_col ? std::fabs(d) > opt_tol : (bs.atup[j] ? d > opt_tol : d < -opt_tol)) viol.emplace_back(std::fabs(d), static_cast<int32_t>(j));
    }
    for (int64_t i = 0; i < m; ++i) { // non-basic logicals sit at 0: reduced cost -y_i, only '<' rows may move (up)
        if (bs.vstat[n + i] != 0 || !lp.lt[i]) continue;
        const double d = -C.hy[i];
        if (d < -opt_tol) viol.emplace_back(std::fabs(d), static_cast<int32_t>(n + i));
    }
}
// the (up to 2,048) worst violators join the tableau
int bring_in(BandCall &C, const HostLp &lp, pl::BasisState &bs, Epoch &E, std::vector<std::pair<double, int32_t>> &viol, int rounds) {
    hipStream_t s = C.s;
    TbState &hst = E.hst;
    const int64_t mp = E.mp;
    std::sort(viol.begin(), viol.end(), [](const std::pair<double, int32_t> &a, const std::pair<double, int32_t> &bb) { return a.first > bb.first || (a.first == bb.first && a.second < bb.second); });
    const int64_t take = std::min<int64_t>(static_cast<int64_t>(viol.size()), 2048);
    if (E.nJ + take > E.sl.cap) { // (nothing is pending here: the run stopped, its batch was folded)
        const int rc_ = E.sl.reserve(s, mp, E.nJ + take + std::max<int64_t>(512, E.nJ / 2), E.nJ);
        if (rc_ != SX_OK) return rc_;
        C.peak_bytes = std::max(C.peak_bytes, 2 * TbSlots::bytes_for(mp, E.nJ) + sizeof(double) * static_cast<size_t>(mp) * (E.EPOCH + 1));
    }
    std::vector<int32_t> add(static_cast<size_t>(take));
    for (int64_t t = 0; t < take; ++t) add[t] = viol[t].second;
    std::sort(add.begin(), add.end());
    for (int32_t v : add)
        if (v >= C.n) bs.xlog[v - C.n] = 0.0;
    SX_TRY(load_slots(C, lp, bs, E, E.nJ, add));
    SX_TRY(build_cols(C, E, E.nJ, take, hst.n_eta));
    E.nJ += take;
    C.added_total += take;
    hst.status = 0;
    SX_HIP(hipMemcpyAsync(C.d_st, &hst, sizeof(hst), hipMemcpyHostToDevice, s)); // (status only changed; counters as read)
    SX_HIP(hipStreamSynchronize(s));
    if (C.trace) fprintf(stderr, "[sx_crossover_band]   round %d: %lld columns brought into the tableau by %.1f ms\n", rounds, (long long)take, C.ms());
    return SX_OK;
}
// rounds of "pivot until no tracked column prices out, then price all the others and bring the violators in" until the
// epoch ends: optimal or infeasible over all columns, unbounded, out of iterations, numerical trouble -- or the eta file
// is full (E.restart)
int simplex_rounds(BandCall &C, const HostLp &lp, pl::BasisState &bs, Epoch &E) {
    TbState &hst = E.hst;
    int rounds = 0;
    std::vector<std::pair<double, int32_t>> viol;
    for (;;) {
        ++rounds;
        SX_TRY(run_pivots(C, E));
        if (C.trace)
            fprintf(stderr, "[sx_crossover_band]   round %d: status %d after %lld iterations (%lld pivots, %lld flips, %lld of no length), phase %d, %d "
                            "infeasible (sum %.3e), %.1f ms so far\n", rounds, hst.status, hst.iters, hst.pivots, hst.flips, hst.degen, hst.phase,
                    hst.n_inf, hst.sum_inf, C.ms());
        if (hst.status == 3 && hst.n_eta >= hst.cap_eta && C.tot_iters + hst.iters < C.max_iter) {
            E.restart = true; // the eta file is full: factor the basis afresh
            break;
        }
        if (hst.status != 1) break;
        const bool ph1 = hst.phase == 1;
        SX_TRY(price_all(C, bs, E, rounds, ph1));
        violators(C, lp, bs, E, viol);
        if (C.trace) fprintf(stderr, "[sx_crossover_band]   round %d (%s): %zu columns outside the tableau price out\n", rounds, ph1 ? "phase 1" : "phase 2", viol.size());
        if (viol.empty()) {
            if (ph1) hst.status = 101; // infeasible: no column anywhere reduces the infeasibility
            break;
        }
        SX_TRY(bring_in(C, lp, bs, E, viol, rounds));
    }
    return SX_OK;
}

// the epoch's end state -> host: the basic set, the tracked columns and the point as the device left them
int end_state(BandCall &C, const HostLp &lp, pl::BasisState &bs, Epoch &E) {
    hipStream_t s = C.s;
    const int64_t n = C.n, mp = E.mp, nJ = E.nJ;
    SX_TRY(down(s, E.hh, E.d_head, static_cast<size_t>(mp)));
    SX_TRY(down(s, E.hxb, E.d_xB, static_cast<size_t>(mp)));
    SX_TRY(down(s, E.hvarJ, E.sl.varJ, static_cast<size_t>(nJ)));
    SX_TRY(down(s, E.hstatJ, E.sl.statJ, static_cast<size_t>(nJ)));
    SX_TRY(down(s, E.hxJ, E.sl.xJ, static_cast<size_t>(nJ)));
    SX_HIP(hipStreamSynchronize(s));
    C.tot_iters += E.hst.iters;
    C.tot_pivots += E.hst.pivots;
    C.tot_flips += E.hst.flips;
    C.tot_degen += E.hst.degen;
    vstat_from_device(E.hh, E.hvarJ, &E.hstatJ, bs.vstat);
    C.viol_max = basic_values_to_point(lp, E.hh, E.hxb, bs.hx);
    std::fill(bs.is_basic.begin(), bs.is_basic.end(), 0);
    bs.prev_pos.assign(static_cast<size_t>(E.g.m1_all), -1);
    for (int64_t p = 0; p < mp; ++p) {
        const int64_t v = E.hh[p];
        if (v < 0) continue;
        bs.is_basic[v] = 1;
        if (p < E.g.m1 && v == E.head[p] && E.g.old_of_new[p] >= 0) bs.prev_pos[E.g.old_of_new[p]] = v;
    }
    bs.tracked.clear();
    for (int64_t t = 0; t < nJ; ++t) {
        const int64_t v = E.hvarJ[t];
        bs.tracked.push_back(static_cast<int32_t>(v));
        if (v < n) {
            bs.hx[v] = E.hxJ[t];
            bs.atup[v] = E.hstatJ[t] == TB_UPP;
        }
    }
    C.final_status = E.hst.status;
    return SX_OK;
}

// The vertex against A itself before it is called optimal: x_B was only ever updated, y came through the eta
// file -- row residuals of x (one K2 walk) and the reduced costs of the basic columns (they are in E.hrc).
// ok = false: beyond the tolerances (the driver factors the current basis afresh and goes on from there, twice at most)
int check_vertex(BandCall &C, const HostLp &lp, pl::BasisState &bs, Epoch &E, bool &ok) {
    hipStream_t s = C.s;
    const int64_t m = C.m, n = C.n, mp = E.mp;
    SX_TRY(slack_to_host(C, bs.hx, C.hslack));
    C.resid_max = row_residual(lp, C.hslack);
    if (C.resid_max > 1e-11) {
        // one step of iterative refinement with the factors at hand: B delta = b - A x - s (s: the logicals'
        // values), x_B += delta -- what thousands of updates x_B -= theta alpha left behind goes at once
        std::vector<double> slog(static_cast<size_t>(m), 0.0), rr(static_cast<size_t>(mp), 0.0), delta;
        for (int64_t p = 0; p < mp; ++p)
            if (E.hh[p] >= n) slog[E.hh[p] - n] = E.hxb[p];
        for (int64_t t = 0; t < E.nJ; ++t)
            if (E.hvarJ[t] >= n) slog[E.hvarJ[t] - n] = E.hxJ[t];
        for (int64_t i = 0; i < m; ++i) rr[E.g.eqidx[i]] = C.hslack[i] - slog[i];
        SX_TRY(up(s, E.d_vec, rr));
        SX_TRY(ftran_cols(C, E, E.d_vec, 1, E.hst.n_eta, false));
        SX_TRY(down(s, delta, E.d_vec, static_cast<size_t>(mp)));
        SX_HIP(hipStreamSynchronize(s));
        for (int64_t p = 0; p < mp; ++p)
            if (E.hh[p] >= 0) E.hxb[p] += delta[p];
        C.viol_max = basic_values_to_point(lp, E.hh, E.hxb, bs.hx);
        SX_TRY(slack_to_host(C, bs.hx, C.hslack));
        const double before = C.resid_max;
        C.resid_max = row_residual(lp, C.hslack);
        if (C.trace) fprintf(stderr, "[sx_crossover_band] refinement of x_B: row residual %.2e -> %.2e (relative), bound violation %.2e\n", before, C.resid_max, C.viol_max);
    }
    double rc_basic = 0.0;
    if (static_cast<int64_t>(E.hrc.size()) == n)
        for (int64_t j = 0; j < n; ++j)
            if (bs.vstat[j] == 1) rc_basic = std::max(rc_basic, std::fabs(E.hrc[j]) / (1.0 + std::fabs(lp.c[j])));
    if (C.trace) fprintf(stderr, "[sx_crossover_band] check of the vertex: row residual %.2e (relative), reduced costs of basic columns %.2e\n", C.resid_max, rc_basic);
    ok = !(C.resid_max > 10.0 * C.feas_tol || rc_basic > 10.0 * C.opt_tol || C.viol_max > 10.0 * C.feas_tol);
    return SX_OK;
}

int outputs(BandCall &C, const HostLp &lp, const pl::BasisState &bs, double *x_out, double *y_out, int8_t *vbasis_out, int8_t *cbasis_out,
            sx_simplex_result *result) {
    hipStream_t s = C.s;
    const int64_t m = C.m, n = C.n;
    std::vector<int8_t> vb(static_cast<size_t>(n)), cb(static_cast<size_t>(m), -1);
    // (a non-basic free column sits at no bound: -3, the code it is read with on entry)
    for (int64_t j = 0; j < n; ++j)
        vb[j] = bs.vstat[j] == 1 ? 0 : ((bs.vstat[j] == 3 || (std::isinf(lp.l[j]) && std::isinf(lp.u[j]))) ? -3 : (bs.atup[j] ? -2 : -1));
    for (int64_t i = 0; i < m; ++i)
        if (bs.vstat[n + i] == 1) cb[i] = 0;
    double obj = 0.0;
    for (int64_t j = 0; j < n; ++j) obj += lp.c[j] * bs.hx[j];
    if (x_out) SX_HIP(hipMemcpyAsync(x_out, bs.hx.data(), sizeof(double) * static_cast<size_t>(n), hipMemcpyHostToDevice, s));
    if (y_out) SX_HIP(hipMemcpyAsync(y_out, C.hy.data(), sizeof(double) * static_cast<size_t>(m), hipMemcpyHostToDevice, s));
    if (vbasis_out) SX_HIP(hipMemcpyAsync(vbasis_out, vb.data(), static_cast<size_t>(n), hipMemcpyHostToDevice, s));
    if (cbasis_out) SX_HIP(hipMemcpyAsync(cbasis_out, cb.data(), static_cast<size_t>(m), hipMemcpyHostToDevice, s));
    SX_HIP(hipStreamSynchronize(s));
    result->status = C.final_status == 1 ? 0 : (C.final_status == 101 ? 1 : C.final_status);
    result->iters = C.tot_iters;
    result->phase1_iters = C.added_total;
    result->warm_start_used = C.given ? 1 : 0;
    result->obj = obj;
    result->max_violation = std::max(C.viol_max > 0 ? C.viol_max : 0.0, C.resid_max);
    if (C.trace)
        fprintf(stderr, "[sx_crossover_band] done: status %lld, %lld iterations (%lld pivots, %lld flips, %lld of no length) in %d epochs, %lld columns added by "
                        "pricing, objective %.12e, max violation %.2e, largest blocks %.2f GB, %.1f ms\n", (long long)result->status, C.tot_iters, C.tot_pivots, C.tot_flips,
                C.tot_degen, C.epochs, (long long)C.added_total, obj, result->max_violation, static_cast<double>(C.peak_bytes) * 1e-9, C.ms());
    return SX_OK;
}

// One entry for the three ways the sparse crossover is started: from the first-order point alone (vbasis_in == NULL: the
// basis is guessed from the margins), or from a given basis (the reference's warm-started final solve,
// lp_methods/algorithms.py:69-74; sx_crossover_band_dev passes NULL).  The control flow and nothing else: every stage is a
// function above, the host set-up between them is sx_band_plan.h.
int crossover_band_impl(sx_ctx *ctx, const sx_matrix *A, const double *b, const double *c, const double *l,
                        const double *u, const uint8_t *row_is_lt, const double *x_start, const int8_t *vbasis_in,
                        const int8_t *cbasis_in, int64_t max_iter, double feas_tol, double opt_tol, double *x_out,
                        double *y_out, int8_t *vbasis_out, int8_t *cbasis_out, sx_simplex_result *result, bool probe_only) {
    SX_ENTER(ctx);
    SX_REQUIRE(A && b && c && l && u && x_start && result, "NULL argument");
    SX_REQUIRE((vbasis_in == nullptr) == (cbasis_in == nullptr), "vbasis_in and cbasis_in come together");
    SX_REQUIRE(A->csr_ptr && A->csc_ptr, "the sparse crossover needs both layouts of A");
    SX_REQUIRE(A->m > 0 && A->n > 0 && A->m + A->n < 2000000000LL, "problem size");
    BandCall C;
    C.ctx = ctx;
    C.A = A;
    C.b = b;
    C.c = c;
    C.s = ctx->stream;
    C.trace = getenv("SX_SPX_TRACE") != nullptr;
    C.given = vbasis_in != nullptr;
    C.t_begin = BandCall::now();
    C.m = A->m;
    C.n = A->n;
    C.max_iter = max_iter > 0 ? max_iter : 50 * (A->m + A->n);
    C.feas_tol = feas_tol > 0 ? feas_tol : 1e-7;
    C.opt_tol = opt_tol > 0 ? opt_tol : 1e-7;
    if (getenv("SX_BAND_PIVTOL_B")) C.tol_band_guess = atof(getenv("SX_BAND_PIVTOL_B"));
    if (getenv("SX_BAND_PIVTOL_S")) C.tol_schur_guess = atof(getenv("SX_BAND_PIVTOL_S"));
    *result = sx_simplex_result{};
    result->status = 4;
    // ---- 1. probe shortcut
    if (probe_only && !vbasis_in) {
        bool taken = false;
        SX_TRY(probe_shortcut(C, taken));
        if (taken) {
            result->status = 0;
            return SX_OK;
        }
    }
    // ---- 2. host copies; 3. plan: rows, the first basic set, the call's blocks
    HostLp lp;
    pl::RowPlan rp;
    pl::BasisState bs;
    SX_TRY(host_copies(C, l, u, row_is_lt, x_start, vbasis_in, cbasis_in, lp, bs));
    SX_TRY(plan_rows(C, lp, rp));
    SX_TRY(first_basic_set(C, lp, rp, x_start, bs));
    SX_TRY(call_blocks(C, static_cast<int64_t>(rp.rows_dense.size()), bs.tracked.size()));
    // ---- 4. epochs: factor the basic set, run the simplex on it; three ways of going round again
    for (;;) {
        ++C.epochs;
        // the basic set is a guess from the margins of the point -- or a given basis whose basic solution turned out far
        // outside the bounds (below): the LUs then set aside what is all but dependent
        const bool guessed = (C.epochs == 1 && !vbasis_in) || C.strict_next;
        C.strict_next = false;
        Epoch E; // this epoch's device arrays and factors
        pl::match_columns_to_rows(lp.csc(), rp, bs.is_basic, bs.prev_pos, E.mt);
        if (C.trace) fprintf(stderr, "[sx_crossover_band] epoch %d: columns matched to rows at %.1f ms\n", C.epochs, C.ms());
        SX_TRY(epoch_geometry(C, lp, rp, E));
        if (probe_only) { // (sx_crossover_band_probe_dev: the matched basis is a band the LU takes -- that was the question)
            result->status = 0;
            return SX_OK;
        }
        SX_TRY(factor_band(C, E, guessed));
        SX_TRY(make_border(C, lp, bs, E, guessed));
        SX_TRY(schur_complement(C, bs, E, guessed));
        SX_TRY(border_blocks(C, lp, E));
        SX_TRY(epoch_arrays(C, bs, E));
        SX_TRY(values_and_rhs(C, lp, bs, E));
        if (vbasis_in && C.epochs == 1 && !C.strict_tried) { // (1) a given basis that is no basis to start from
            bool far = false;
            SX_TRY(given_basis_is_far(C, lp, E, far));
            C.strict_tried = true;
            if (far) {
                C.strict_next = true;
                continue;
            }
        }
        if (C.trace) SX_TRY(trace_basic_solution(C, lp, bs, E));
        SX_TRY(tableau_columns(C, lp, bs, E));
        SX_TRY(simplex_rounds(C, lp, bs, E));
        SX_TRY(end_state(C, lp, bs, E));
        if (E.restart) continue; // (2) the eta file is full ...
        if ((E.hst.status == 4 || E.hst.status == 2) && C.bad_epochs < 2 && C.tot_iters < C.max_iter) { // ... or a tiny pivot / a ray that should not be: fresh factors first
            ++C.bad_epochs;
            continue;
        }
        if (E.hst.status == 1) { // (3) a vertex that fails the check against A
            bool ok = true;
            SX_TRY(check_vertex(C, lp, bs, E, ok));
            if (!ok) {
                if (C.check_epochs < 2 && C.tot_iters < C.max_iter) {
                    ++C.check_epochs;
                    continue;
                }
                C.final_status = 4;
            }
        }
        break;
    }
    // ---- 5. outputs
    return outputs(C, lp, bs, x_out, y_out, vbasis_out, cbasis_out, result);
}

} // namespace

SX_API int sx_crossover_band_basis_dev(sx_ctx *ctx, const sx_matrix *A, const double *b, const double *c, const double *l,
                                       const double *u, const uint8_t *row_is_lt, const double *x_start, const int8_t *vbasis_in,
                                       const int8_t *cbasis_in, int64_t max_iter, double feas_tol, double opt_tol, double *x_out,
                                       double *y_out, int8_t *vbasis_out, int8_t *cbasis_out, sx_simplex_result *result) {
    return crossover_band_impl(ctx, A, b, c, l, u, row_is_lt, x_start, vbasis_in, cbasis_in, max_iter, feas_tol, opt_tol, x_out, y_out, vbasis_out,
                               cbasis_out, result, false);
}

// Would the sparse crossover take this LP from this point?  Runs its set-up up to the band-width check -- host copies, row
// order, the basic set guessed from x_start, matching -- and nothing else: SX_OK / SX_ERR_UNSUPPORTED.  A backend asks before
// it sizes its first-order stage (the dense crossover needs four times the iterations in front of it).
SX_API int sx_crossover_band_probe_dev(sx_ctx *ctx, const sx_matrix *A, const double *b, const double *c, const double *l,
                                       const double *u, const uint8_t *row_is_lt, const double *x_start) {
    sx_simplex_result r{};
    return crossover_band_impl(ctx, A, b, c, l, u, row_is_lt, x_start, nullptr, nullptr, 0, 0.0, 0.0, nullptr, nullptr, nullptr, nullptr, &r, true);
}

SX_API int sx_crossover_band_dev(sx_ctx *ctx, const sx_matrix *A, const double *b, const double *c, const double *l,
                                 const double *u, const uint8_t *row_is_lt, const double *x_start, int64_t max_iter,
                                 double feas_tol, double opt_tol, double *x_out, double *y_out, int8_t *vbasis_out,
                                 int8_t *cbasis_out, sx_simplex_result *result) {
    return sx_crossover_band_basis_dev(ctx, A, b, c, l, u, row_is_lt, x_start, nullptr, nullptr, max_iter, feas_tol, opt_tol, x_out, y_out,
                                       vbasis_out, cbasis_out, result);
}
