// Entropic OT warm start in the log domain: the variant of the step the reference's driver runs before the OT
// crossover (scripts/run_network_crossover.py:95-101, POT's `sinkhorn`) that still works when exp(-M/reg) leaves
// the range of a double -- image pairs restricted to their non-zero pixels with a reg of a few thousandths, where
// sx_sinkhorn.hip breaks down at iteration 0.  The algorithm is POT's published `sinkhorn_log` (POT is absent and
// unpinned: parity unpinned, tests/test_gpu_sinkhorn_log.py restates it in extended precision):
//
//   Mr = M / (-reg);  u = 0[S], v = 0[D]                    (log-scalings; log a_i = -inf marks a zero-mass point)
//   repeat:  v = log b - LSE_i (Mr[i, :] + u[i]);   u = log a - LSE_j (Mr[:, j] + v[j])
//            every 10th iteration (0, 10, ...):  err = || sum_i exp(Mr + u_i + v_j) - b ||_2 ;  stop when err < stopThr
//   plan = exp(Mr + u_i + v_j)
//
// One set of kernels serves sx_sinkhorn_log_dev (B = 1) and sx_sinkhorn_log_batch_dev (B <= 16 over one M).
//
// Reduction.  A log-sum-exp is carried as a pair (m, s) = (maximum so far, sum of exp(x - m)).  Both passes use the
// ONLINE form: a new term t costs one exp, exp(-|t - m|), which is the term's weight when t <= m and the factor that
// rescales s when t moves the maximum -- so every matrix element costs exactly one exp per pass whether or not the
// maximum moves, and nothing is held back for a second sweep.  The two-sweep form (maximum first, then the sum over
// values kept in registers) was not taken because neither a slice of rows nor a lane's share of a row has a length
// that registers bound.  Two pairs merge with one exp (of the smaller maximum's offset); (-inf, 0) is the identity
// and no path forms -inf - (-inf).
//
// Column pass (k_sl_cols + k_sl_cols_finish): lanes along the columns, so a wave reads 64 consecutive doubles of a
// row of Mr; the rows are cut into slices by the rule of sx_sinkhorn.hip (4 * clamp(ceil(S / 128), 1, 16) slices,
// a function of S alone), each lane reduces its slice to a pair, the finish merges a column's pairs in ascending
// slice order.  Row pass (k_sl_rows): one wave per row, lanes strided over the columns, each lane its own pair,
// the 64 pairs merged by a fixed shuffle tree (offsets 32, 16, ..., 1), lane 0 writes.  No atomics anywhere: a run
// repeats bit for bit.
//
// Stopping test.  The column sums of the plan are exp(v_j + LSE_i (Mr_ij + u_i)), and that LSE is the first half of
// the NEXT iteration's v.  So the test of iteration ii is evaluated by the column finish of iteration ii + 1 from
// the value it computes anyway; v is double-buffered by iteration parity so that an instance that turns out to have
// converged keeps the v it was tested with.  A tested iteration costs one one-block launch (k_sl_verdict) more,
// never a third reduction.  When the last iteration is a tested one, one column pass follows the loop.
//
// Batched form.  Log-scalings are instance-minor in groups of NB = 4 instances: a lane loads an element of Mr once
// and carries four pairs; the groups are the z-dimension of the grids and re-read Mr from cache.  Sixteen pairs per
// lane fit the register file, but 784 columns x 28 slices are 364 waves on 1,024 SIMDs: a wave has a SIMD to itself
// and waits on its own exp chain, while the 4.9 MB matrix sits in L2 / Infinity Cache, so instances were given extra
// waves before extra work per wave (reasoned from those counts; sixteen pairs per lane was not built and timed
// against it -- profiles/r06/sinkhorn_log.md has what was measured).  Instances stop independently (per-instance done flags);
// a zero mass takes its point out of an instance (log-scaling -inf from the start, plan entries exactly 0).
//
// No matrix cores: the reduction is not a contraction -- the stabiliser m differs per output and per instance, and
// exp sits between the load and the sum -- so there is no MFMA shape here, for one instance or for sixteen.
#include "sx_graph.h"
#include "sx_internal.h"
#include "sx_segwalk.h"

#include <cmath>

namespace {

constexpr int SLB = 16; // instances per call

struct SlState {
    long long iters[SLB];
    int done[SLB]; // 1 converged, 2 tested err not finite, 3 padding instance (never iterates)
    double err[SLB];
};

struct SlPair {
    double m, s;
};

// (m, s) <- (m, s) + the single term t: one exp; t = -inf adds nothing, also to the empty pair
__device__ __forceinline__ void sl_add(double &m, double &s, double t) {
    const double e = exp(-fabs(t - m));
    const bool up = t > m;
    s = up ? s * e + 1.0 : (t == -INFINITY ? s : s + e);
    m = up ? t : m;
}

// (m, s) <- (m, s) + (m2, s2): one exp, of the smaller maximum's offset
__device__ __forceinline__ void sl_merge(double &m, double &s, double m2, double s2) {
    const double e = exp(-fabs(m2 - m));
    const bool up = m2 > m;
    s = up ? s * e + s2 : (m2 == -INFINITY ? s : s + s2 * e);
    m = up ? m2 : m;
}

// Mr = M / (-reg);  log-marginals into the grouped instance-minor layout X[g][r][NB];  u and both v buffers start at 0
// on the support and at -inf off it -- POT's start on the problem restricted to the support, so that the iterates ARE
// those of the restricted problem from the first column pass on
template <int NB>
__global__ __launch_bounds__(SX_WG) void k_sl_init(SlState *st, int64_t S, int64_t D, int B, int groups,
                                                   const double *__restrict__ a, const double *__restrict__ b,
                                                   const double *__restrict__ M, double reg, double *__restrict__ Mr,
                                                   double *__restrict__ loga, double *__restrict__ logb,
                                                   double *__restrict__ U, double *__restrict__ V) {
    const int64_t n = S * D, nS = S * NB * groups, nD = D * NB * groups;
    const int64_t top = n > nS ? (n > nD ? n : nD) : (nS > nD ? nS : nD);
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; e < top;
         e += static_cast<int64_t>(gridDim.x) * SX_WG) {
        if (e < n) Mr[e] = M[e] / (-reg);
        const int64_t r = (e / NB) % S, rd = (e / NB) % D;
        const int cs = static_cast<int>(e / (NB * S)) * NB + static_cast<int>(e % NB);
        const int cd = static_cast<int>(e / (NB * D)) * NB + static_cast<int>(e % NB);
        if (e < nS) {
            const double la = (cs < B) ? log(a[static_cast<int64_t>(cs) * S + r]) : -INFINITY;
            loga[e] = la;
            U[e] = (la == -INFINITY) ? -INFINITY : 0.0;
        }
        if (e < nD) {
            const double lb = (cd < B) ? log(b[static_cast<int64_t>(cd) * D + rd]) : -INFINITY;
            logb[e] = lb;
            V[e] = V[nD + e] = (lb == -INFINITY) ? -INFINITY : 0.0;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < SLB) {
        st->iters[threadIdx.x] = 0;
        st->done[threadIdx.x] = (static_cast<int>(threadIdx.x) < B) ? 0 : 3;
        st->err[threadIdx.x] = 1.0;
    }
}

// part[g][slice][j][c] = the pair of LSE over the rows i of the slice of (Mr[i][j] + U[g][i][c])
template <int NB>
__global__ __launch_bounds__(SX_WG) void k_sl_cols(const SlState *st, int64_t S, int64_t D,
                                                   const double *__restrict__ Mr, const double *__restrict__ U,
                                                   SlPair *__restrict__ part) {
    const int g = blockIdx.z;
    bool live[NB], any = false;
#pragma unroll
    for (int c = 0; c < NB; ++c) any |= (live[c] = st->done[g * NB + c] == 0);
    if (!any) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t j = static_cast<int64_t>(blockIdx.x) * 64 + lane;
    const int64_t slice = static_cast<int64_t>(blockIdx.y) * (SX_WG / 64) + wave;
    const int64_t nslices = static_cast<int64_t>(gridDim.y) * (SX_WG / 64);
    if (j >= D) return;
    const int64_t rows = (S + nslices - 1) / nslices;
    const int64_t i0 = slice * rows, i1 = (i0 + rows < S) ? i0 + rows : S;
    const double *__restrict__ Ug = U + static_cast<int64_t>(g) * S * NB;
    double m[NB], s[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) m[c] = -INFINITY, s[c] = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
        const double x = Mr[i * D + j];
#pragma unroll
        for (int c = 0; c < NB; ++c)
            if (live[c]) sl_add(m[c], s[c], x + Ug[i * NB + c]);
    }
    SlPair *__restrict__ out = part + ((static_cast<int64_t>(g) * nslices + slice) * D + j) * NB;
#pragma unroll
    for (int c = 0; c < NB; ++c) out[c] = SlPair{m[c], s[c]};
}

// one lane per (column j, instance c) of group g: L = LSE over all rows, the slice pairs merged in ascending order;
// Vnew = log b - L;  with `test`, err_part[g][block][c] = sum over the block's columns of (exp(Vold + L) - b)^2 --
// the marginal violation of the pair (u, Vold) that the previous iteration left
template <int NB>
__global__ __launch_bounds__(SX_WG) void k_sl_cols_finish(const SlState *st, int64_t D, int64_t nslices,
                                                          const SlPair *__restrict__ part,
                                                          const double *__restrict__ logb,
                                                          const double *__restrict__ Vold, double *__restrict__ Vnew,
                                                          int test, double *__restrict__ err_part) {
    const int g = blockIdx.y;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; // = j * NB + c
    const int c = static_cast<int>(e % NB);
    const bool active = e < D * NB && st->done[g * NB + c] == 0;
    double sq = 0.0;
    if (active) {
        const int64_t ge = static_cast<int64_t>(g) * D * NB + e;
        double m = -INFINITY, s = 0.0;
        for (int64_t q = 0; q < nslices; ++q) {
            const SlPair p = part[(static_cast<int64_t>(g) * nslices + q) * D * NB + e];
            sl_merge(m, s, p.m, p.s);
        }
        const double L = (s > 0.0) ? m + log(s) : -INFINITY;
        const double lb = logb[ge];
        Vnew[ge] = (lb == -INFINITY) ? -INFINITY : lb - L;
        if (test) {
            const double d = exp(Vold[ge] + L) - exp(lb);
            sq = d * d;
        }
    }
    if (test) { // uniform.  Per instance: lanes c, c + NB, ... of a wave by a fixed tree, then the waves in order
        __shared__ double ws[SX_WG / 64][NB];
#pragma unroll
        for (int o = 32; o >= NB; o >>= 1) sq += __shfl_down(sq, o, 64);
        const int lane = threadIdx.x & 63;
        if (lane < NB) ws[threadIdx.x >> 6][lane] = sq;
        __syncthreads();
        if (threadIdx.x < NB) {
            double t = ws[0][threadIdx.x];
            for (int w = 1; w < SX_WG / 64; ++w) t += ws[w][threadIdx.x];
            err_part[(static_cast<int64_t>(g) * gridDim.x + blockIdx.x) * NB + threadIdx.x] = t;
        }
    }
}

// one lane per instance: close the stopping test whose partial sums the column finish has just written
template <int NB>
__global__ void k_sl_verdict(SlState *st, const double *__restrict__ err_part, int nparts, double stop_thr) {
    const int c = threadIdx.x;
    if (c >= SLB || st->done[c] != 0) return;
    const double *p = err_part + static_cast<int64_t>(c / NB) * nparts * NB + (c % NB);
    double t = 0.0;
    for (int k = 0; k < nparts; ++k) t += p[static_cast<int64_t>(k) * NB];
    const double err = sqrt(t);
    st->err[c] = err;
    if (err < stop_thr) st->done[c] = 1;
    else if (!(fabs(err) < INFINITY)) st->done[c] = 2;
}

// U[g][i][c] = log a - LSE over the columns j of (Mr[i][j] + V[g][j][c])    (one wave per row); counts the iteration
template <int NB>
__global__ __launch_bounds__(SX_WG) void k_sl_rows(SlState *st, int64_t S, int64_t D, const double *__restrict__ Mr,
                                                   const double *__restrict__ loga, const double *__restrict__ V,
                                                   double *__restrict__ U) {
    const int g = blockIdx.y;
    bool live[NB], any = false;
#pragma unroll
    for (int c = 0; c < NB; ++c) any |= (live[c] = st->done[g * NB + c] == 0);
    if (!any) return;
    if (blockIdx.x == 0 && threadIdx.x < NB && live[threadIdx.x]) st->iters[g * NB + threadIdx.x] += 1;
    const int lane = threadIdx.x & 63;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (SX_WG / 64) + (threadIdx.x >> 6);
    if (i >= S) return;
    const double *__restrict__ Vg = V + static_cast<int64_t>(g) * D * NB;
    double m[NB], s[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) m[c] = -INFINITY, s[c] = 0.0;
    for (int64_t j = lane; j < D; j += 64) {
        const double x = Mr[i * D + j];
#pragma unroll
        for (int c = 0; c < NB; ++c)
            if (live[c]) sl_add(m[c], s[c], x + Vg[j * NB + c]);
    }
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        if (!live[c]) continue; // uniform
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double m2 = __shfl_down(m[c], o, 64), s2 = __shfl_down(s[c], o, 64);
            sl_merge(m[c], s[c], m2, s2);
        }
        if (lane == 0) {
            const int64_t ge = (static_cast<int64_t>(g) * S + i) * NB + c;
            const double la = loga[ge];
            U[ge] = (la == -INFINITY || !(s[c] > 0.0)) ? -INFINITY : la - (m[c] + log(s[c]));
        }
    }
}

// plans[c][i][j] = exp(Mr[i][j] + u_c[i] + v_c[j]), v_c from the buffer instance c wrote last; also unpacks the
// log-scalings into the caller's instance-major arrays
template <int NB>
__global__ __launch_bounds__(SX_WG) void k_sl_plan(const SlState *st, int64_t S, int64_t D, int B, int groups,
                                                   const double *__restrict__ Mr, const double *__restrict__ U,
                                                   const double *__restrict__ V, double *__restrict__ plans,
                                                   double *__restrict__ logu_out, double *__restrict__ logv_out) {
    const int64_t n = S * D, nD = D * NB * groups;
    const int64_t top = n > S ? (n > D ? n : D) : (S > D ? S : D);
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; e < top;
         e += static_cast<int64_t>(gridDim.x) * SX_WG) {
        const int64_t i = e / D, j = e - i * D;
        const double x = (e < n) ? Mr[e] : 0.0;
        for (int c = 0; c < B; ++c) {
            const int g = c / NB, k = c % NB;
            const double *__restrict__ Vc = V + (((st->iters[c] - 1) & 1) ? nD : 0) + static_cast<int64_t>(g) * D * NB + k;
            const double *__restrict__ Uc = U + static_cast<int64_t>(g) * S * NB + k;
            if (plans && e < n) plans[static_cast<int64_t>(c) * n + e] = exp(x + Uc[i * NB] + Vc[j * NB]);
            if (logu_out && e < S) logu_out[static_cast<int64_t>(c) * S + e] = Uc[e * NB];
            if (logv_out && e < D) logv_out[static_cast<int64_t>(c) * D + e] = Vc[e * NB];
        }
    }
}

inline unsigned grid1d(int64_t n, int64_t cap = 4096) {
    int64_t g = (n + SX_WG - 1) / SX_WG;
    if (g > cap) g = cap;
    return static_cast<unsigned>(g < 1 ? 1 : g);
}

template <int NB>
int sl_run(sx_ctx *ctx, int64_t S, int64_t D, int B, const double *a, const double *b, const double *M, double reg,
           int64_t max_iter, double stop_thr, double *plans, double *logu_out, double *logv_out,
           sx_sinkhorn_result *results) {
    hipStream_t s = ctx->stream;
    const int groups = (B + NB - 1) / NB;
    int64_t ysl = (S + 127) / 128;
    ysl = ysl < 1 ? 1 : (ysl > 16 ? 16 : ysl);
    const int64_t nslices = ysl * (SX_WG / 64);
    const size_t uS = static_cast<size_t>(S), uD = static_cast<size_t>(D);
    const size_t nS = uS * NB * groups, nD = uD * NB * groups;
    const unsigned gF = static_cast<unsigned>((D * NB + SX_WG - 1) / SX_WG);
    // workspace: state | Mr[S*D] | loga U [nS] | logb V V' [nD] | err_part[groups*gF*NB] | part[nslices*nD] pairs
    const size_t bytes = 1024 + sizeof(double) * (uS * uD + 2 * nS + 3 * nD + static_cast<size_t>(groups) * gF * NB +
                                                  2 * static_cast<size_t>(nslices) * nD) + 64;
    SX_TRY(sx_reserve2(ctx, bytes));
    char *base = static_cast<char *>(ctx->ws2);
    SlState *st = reinterpret_cast<SlState *>(base); // sizeof(SlState) = 320
    double *Mr = reinterpret_cast<double *>(base + 1024);
    double *loga = Mr + uS * uD, *U = loga + nS, *logb = U + nS, *V = logb + nD;
    double *err_part = V + 2 * nD;
    SlPair *part = reinterpret_cast<SlPair *>(err_part + static_cast<size_t>(groups) * gF * NB);
    hipLaunchKernelGGL(k_sl_init<NB>, dim3(grid1d(S * D)), dim3(SX_WG), 0, s, st, S, D, B, groups, a, b, M, reg, Mr, loga,
                       logb, U, V);
    const dim3 gc(static_cast<unsigned>((D + 63) / 64), static_cast<unsigned>(ysl), static_cast<unsigned>(groups));
    const dim3 gf(gF, static_cast<unsigned>(groups));
    const dim3 gr(static_cast<unsigned>((S + SX_WG / 64 - 1) / (SX_WG / 64)), static_cast<unsigned>(groups));

    // iteration ii writes v into buffer ii & 1 and closes the stopping test of iteration ii - 1 when that was a tested one
    auto columns = [&](int64_t ii) {
        const int test = (ii % 10 == 1);
        double *Vnew = V + ((ii & 1) ? nD : 0), *Vold = V + ((ii & 1) ? 0 : nD);
        hipLaunchKernelGGL(k_sl_cols<NB>, gc, dim3(SX_WG), 0, s, st, S, D, Mr, U, part);
        hipLaunchKernelGGL(k_sl_cols_finish<NB>, gf, dim3(SX_WG), 0, s, st, D, nslices, part, logb, Vold, Vnew, test, err_part);
        if (test) hipLaunchKernelGGL(k_sl_verdict<NB>, dim3(1), dim3(64), 0, s, st, err_part, static_cast<int>(gF), stop_thr);
        return Vnew;
    };
    auto iteration = [&](int64_t ii) {
        const double *Vnew = columns(ii);
        hipLaunchKernelGGL(k_sl_rows<NB>, gr, dim3(SX_WG), 0, s, st, S, D, Mr, loga, Vnew, U);
    };
    // groups of ten iterations (an even count: the buffer parity repeats), captured once and replayed; a linear chain
    SxGraphBatch graph;
    if (max_iter >= 20 && sx_graph_wanted(ctx, 0))
        graph.capture(s, [&]() {
            for (int k = 0; k < 10; ++k) iteration(k);
        });
    (void)hipGetLastError();
    SlState host;
    memset(&host, 0, sizeof(host));
    auto all_done = [&]() {
        for (int c = 0; c < B; ++c)
            if (!host.done[c]) return false;
        return true;
    };
    auto read_state = [&]() {
        return hipGetLastError() == hipSuccess &&
               hipMemcpyAsync(&host, st, sizeof(host), hipMemcpyDeviceToHost, s) == hipSuccess &&
               hipStreamSynchronize(s) == hipSuccess;
    };
    int64_t launched = 0;
    bool ok = true;
    while (ok && launched < max_iter && !all_done()) {
        if (graph.ready() && launched + 10 <= max_iter) {
            ok = graph.launch(s) == hipSuccess;
            launched += 10;
        } else {
            const int64_t upto = (launched + 10 < max_iter) ? launched + 10 : max_iter;
            for (; launched < upto; ++launched) iteration(launched);
        }
        ok = ok && read_state();
    }
    if (ok && max_iter % 10 == 1 && !all_done()) { // the last iteration was a tested one: its test is still open
        columns(max_iter);
        ok = read_state();
    }
    if (!ok) {
        sx_set_error("log-domain Sinkhorn iteration group failed");
        return SX_ERR_HIP;
    }
    hipLaunchKernelGGL(k_sl_plan<NB>, dim3(grid1d(S * D)), dim3(SX_WG), 0, s, st, S, D, B, groups, Mr, U, V, plans, logu_out,
                       logv_out);
    SX_HIP(hipGetLastError());
    SX_HIP(hipStreamSynchronize(s));
    for (int c = 0; c < B; ++c) {
        results[c].iters = host.iters[c];
        results[c].status = host.done[c]; // 0 iteration limit, 1 converged, 2 tested err not finite
        results[c].err = host.err[c];
    }
    return SX_OK;
}

} // namespace

SX_API int sx_sinkhorn_log_dev(sx_ctx *ctx, int64_t S, int64_t D, const double *a, const double *b, const double *M,
                               double reg, int64_t max_iter, double stop_thr, double *plan, double *logu_out,
                               double *logv_out, sx_sinkhorn_result *result) {
    SX_ENTER(ctx);
    SX_REQUIRE(S > 0 && D > 0, "S and D must be positive");
    SX_REQUIRE(a && b && M && result, "NULL argument");
    SX_REQUIRE(reg > 0 && max_iter >= 0, "reg must be positive and max_iter non-negative");
    return sl_run<1>(ctx, S, D, 1, a, b, M, reg, max_iter, stop_thr, plan, logu_out, logv_out, result);
}

SX_API int sx_sinkhorn_log_batch_dev(sx_ctx *ctx, int64_t S, int64_t D, int64_t B, const double *a, const double *b,
                                     const double *M, double reg, int64_t max_iter, double stop_thr, double *plans,
                                     double *logu_out, double *logv_out, sx_sinkhorn_result *results) {
    SX_ENTER(ctx);
    SX_REQUIRE(S > 0 && D > 0, "S and D must be positive");
    SX_REQUIRE(B >= 1 && B <= SLB, "1 <= B <= 16 instances per batch");
    SX_REQUIRE(a && b && M && results, "NULL argument");
    SX_REQUIRE(reg > 0 && max_iter >= 0, "reg must be positive and max_iter non-negative");
    return sl_run<4>(ctx, S, D, static_cast<int>(B), a, b, M, reg, max_iter, stop_thr, plans, logu_out, logv_out, results);
}
