// Log-domain entropic OT warm start on a separable H x W pixel grid: one workgroup per image pair, the whole solve in
// LDS.  The reference builds the cost of its MNIST instances as |dy| + |dx| on the pixel grid (scripts/mnist2ot.py:30-40)
// and its driver runs POT's `sinkhorn` on ten such pairs (scripts/run_network_crossover.py:95-101).  That cost is a
// Kronecker sum  M[(y,x),(y',x')] = Cy[y,y'] + Cx[x,x'],  and a log-sum-exp over it factors into two short ones:
//
//   LSE_{y,x}(-M/reg + z[y,x]) = LSE_y( Ry[y,y'] + T[y,x'] ),   T[y,x'] = LSE_x( Rx[x,x'] + z[y,x] ),   R. = C. / (-reg)
//
// so a half-iteration costs H*W*(H+W) exponentials instead of (H*W)^2 and never touches an n x n array.  The algorithm
// is the one sx_sinkhorn_log.hip states (POT's published `sinkhorn_log`; POT is absent and unpinned: parity unpinned),
// unchanged: log-scalings 0 on an instance's support and -inf off it, v = log b - LSE(u), u = log a - LSE(v), the test
// err = || sum_i plan_ij - b ||_2 at iterations 0, 10, ..., status 0 iteration limit / 1 converged / 2 err not finite.
//
// Work split (k_sg_solve).  blockIdx.x is the instance; 1,024 lanes (16 waves, 4 per SIMD of one CU).  Resident in LDS
// for the whole launch: Rx, Ry, u, v, the intermediate T, and vn (below).  log a and log b do NOT fit beside them at
// 56 x 56 (175 KB), so they live in the call's workspace and an output loads its own once per half-iteration -- one
// load against H or W exponentials; one path for every size was preferred to a second one for small grids.
//   LIMIT:  W*(W|1) + H*(H|1) + 4*H*W  <=  20,000 doubles   (SG_CAP; 160,000 of the CU's 163,840 bytes of LDS)
// 56 x 56 needs 18,928, 17 x 64 needs 8,801, 28 x 28 needs 4,760.  A grid beyond the limit is refused with
// SX_ERR_UNSUPPORTED.  (A smaller array for small grids would not put two workgroups on a CU: the kernel takes 90
// VGPRs, and two groups of 1,024 lanes have 64 each.)
//
// LSE form: TWO SWEEPS, built.  An LSE here has at most max(H, W) terms, so the maximum is taken first (an add and a
// max per term) and the terms exp(t - m) of the second sweep are independent: they pipeline, where the online pair of
// sx_sinkhorn_log.hip chains each exp behind the one before it.  Both sweeps re-read their two operands from LDS (two
// ds_read_b64 per term beside a ~40-instruction fp64 exp) rather than hold 56 terms in registers.  An all -inf input
// gives m = -inf and the result -inf without forming -inf - (-inf).  The online form was NOT built for this kernel and
// is not timed against it; that choice is reasoned from the dependence chains only.
// Several lanes per output, built and timed: P = 2^lp lanes (the high bits of the lane index, so the 64 / P outputs of
// a wave stay consecutive) each take every P-th term; maximum and sum close by an xor butterfly (both partners add the
// same two numbers, so all P lanes hold the same bits).  P does not shorten the work; it spreads a stage with few
// outputs over more waves.  Measured with P forced (profiles/r06/sinkhorn_grid.md), us per iteration at P = 1, 2, 4, 8:
// 12 x 12: 10.5, 9.0, 8.6, 11.6;  28 x 28: 43.9, 39.4, 49.7, 73.1;  56 x 56: 271, 281, 311, 390 -- every output costs
// about 3 exponentials' time beside its terms and every doubling of P about 0.45 more, so P pays only while the CU is
// short of waves.  sg_lanes is fitted to those three sizes: double P until a stage has 24 waves of work, P <= 4.
//
// Layout.  Outputs are always the H x W grid, x fastest along the lanes.  Rx is W rows of W|1 doubles and Ry is H rows
// of H|1: the v-half reads R.[k][out] along a row, the u-half reads R.[out][k] down a column, and with an odd row
// length 32 consecutive rows fall into 32 different 8-byte banks.  No transposed copies: they would not fit at 56 x 56.
//
// Stopping test, closed in the kernel.  The column sums of the plan of (u, v) are exp(v + L) with L = LSE(u), and
// log b - L is the next iteration's v.  A tested iteration computes L once, keeps vn = log b - L in LDS, reduces
// sum (exp(v + L) - b)^2 (lane, then a shuffle tree per wave, then the 16 wave sums in order by lane 0) and, if the
// instance goes on, the next iteration takes vn instead of recomputing it.  No atomics: a run repeats bit for bit.
//
// Bounded launches.  One launch runs at most SG_LAUNCH_ITERS = 100 iterations, then writes u, v, iters, done, err back;
// the host enqueues up to ten launches (finished instances return at once), reads the states, and goes on until
// max_iter or until every instance is done.  numItermax = 1e6 is 10,000 short kernels, never one long one.
//
// No matrix cores: as in sx_sinkhorn_log.hip the stabiliser m differs per output and exp sits between load and sum.
#include "sx_internal.h"

#include <cmath>
#include <vector>

namespace {

constexpr int SG_WG = 1024, SG_WAVES = SG_WG / 64;
constexpr int SG_LAUNCH_ITERS = 100; // iterations per launch; a multiple of 10, so tested iterations open a launch
constexpr int SG_SYNC_LAUNCHES = 10; // launches enqueued between two reads of the states
constexpr int SG_CAP = 20000;        // doubles of LDS for Rx, Ry, u, T, v, vn

struct SgState {
    long long iters;
    int done, pad; // 1 converged, 2 tested err not finite
    double err;
};

struct SgArgs {
    int H, W, lpx, lpy; // log2 of the lanes per output of the LSEs along x and along y (sg_lanes)
    const double *a, *b, *Cy, *Cx;
    double reg, stop_thr;
    double *loga, *logb, *U, *V; // workspace, instance-major [B][H*W]
    SgState *st;
    long long it0, it1; // this launch runs iterations it0 .. it1 - 1
    int first;
};

inline int64_t sg_need(int64_t H, int64_t W) { return W * (W | 1) + H * (H | 1) + 4 * H * W; }

// For every output o = r * W + c of the H x W grid, L = LSE_k( R[k * sk + out * so] + Z[..k..] ) and fin(o, L) on one lane:
// ALONG_X: k runs over x, out = c, the term's Z is Z[r * W + k];  otherwise k runs over y, out = r, Z[k * W + c].
// (sk, so) = (row length, 1) reads R[k][out], (1, row length) reads R[out][k].
template <bool ALONG_X, class Fin>
__device__ __forceinline__ void sg_lse(int H, int W, int lp, const double *R, int sk, int so, const double *Z, Fin fin) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int P = 1 << lp, G = 64 >> lp, p = lane >> (6 - lp), g = lane & (G - 1);
    const int n = H * W, len = ALONG_X ? W : H, zs = ALONG_X ? 1 : W;
    for (int base = wave * G; base < n; base += SG_WAVES * G) { // uniform in a wave: the shuffles below are whole
        const int o = base + g;
        const bool on = o < n;
        const int r = on ? o / W : 0, c = on ? o - r * W : 0;
        const double *Rp = R + (ALONG_X ? c : r) * so;
        const double *Zp = Z + (ALONG_X ? r * W : c);
        double m = -INFINITY;
        for (int k = p; k < len; k += P) m = fmax(m, Rp[k * sk] + Zp[k * zs]);
        for (int off = G; off < 64; off <<= 1) m = fmax(m, __shfl_xor(m, off, 64));
        double s = 0.0;
        if (m != -INFINITY)
            for (int k = p; k < len; k += P) s += exp(Rp[k * sk] + Zp[k * zs] - m);
        for (int off = G; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
        if (on && p == 0) fin(o, (m == -INFINITY) ? -INFINITY : m + log(s));
    }
}

__global__ __launch_bounds__(SG_WG) void k_sg_solve(SgArgs A) {
    __shared__ double lds[SG_CAP];
    __shared__ double red[SG_WAVES];
    __shared__ double s_err;
    __shared__ int s_verdict;
    const int c = blockIdx.x, tid = threadIdx.x;
    const int H = A.H, W = A.W, n = H * W, Wp = W | 1, Hp = H | 1;
    SgState *st = A.st + c;
    if (!A.first && st->done != 0) return; // uniform: the whole workgroup
    double *Rx = lds, *Ry = Rx + W * Wp, *u = Ry + H * Hp, *T = u + n;
    double *v = T + n, *vn = v + n;
    const size_t at = static_cast<size_t>(c) * n;
    const double *loga = A.loga + at, *logb = A.logb + at, *b = A.b + at;
    for (int e = tid; e < W * W; e += SG_WG) Rx[(e / W) * Wp + e % W] = A.Cx[e] / (-A.reg);
    for (int e = tid; e < H * H; e += SG_WG) Ry[(e / H) * Hp + e % H] = A.Cy[e] / (-A.reg);
    double err = 1.0;
    if (A.first) { // POT's start on the instance's own support
        for (int e = tid; e < n; e += SG_WG) {
            const double la = log(A.a[at + e]), lb = log(b[e]);
            A.loga[at + e] = la;
            A.logb[at + e] = lb;
            u[e] = (la == -INFINITY) ? -INFINITY : 0.0;
            v[e] = (lb == -INFINITY) ? -INFINITY : 0.0;
        }
    } else {
        for (int e = tid; e < n; e += SG_WG) u[e] = A.U[at + e], v[e] = A.V[at + e];
        err = st->err;
    }
    __syncthreads();

    int done = 0;
    bool have_vn = false;
    long long ii = A.it0;
    while (ii < A.it1) {
        if (have_vn) { // the test of the iteration before has left v's successor
            double *t = v;
            v = vn, vn = t, have_vn = false;
        } else {
            sg_lse<true>(H, W, A.lpx, Rx, Wp, 1, u, [&](int o, double L) { T[o] = L; });
            __syncthreads();
            sg_lse<false>(H, W, A.lpy, Ry, Hp, 1, T, [&](int o, double L) {
                const double lb = logb[o];
                v[o] = (lb == -INFINITY) ? -INFINITY : lb - L;
            });
            __syncthreads();
        }
        sg_lse<true>(H, W, A.lpx, Rx, 1, Wp, v, [&](int o, double L) { T[o] = L; });
        __syncthreads();
        sg_lse<false>(H, W, A.lpy, Ry, 1, Hp, T, [&](int o, double L) {
            const double la = loga[o];
            u[o] = (la == -INFINITY || L == -INFINITY) ? -INFINITY : la - L;
        });
        __syncthreads();
        const bool test = (ii % 10 == 0);
        ++ii;
        if (!test) continue;
        sg_lse<true>(H, W, A.lpx, Rx, Wp, 1, u, [&](int o, double L) { T[o] = L; });
        __syncthreads();
        double sq = 0.0;
        sg_lse<false>(H, W, A.lpy, Ry, Hp, 1, T, [&](int o, double L) {
            const double lb = logb[o], d = exp(v[o] + L) - b[o];
            vn[o] = (lb == -INFINITY) ? -INFINITY : lb - L;
            sq += d * d;
        });
        for (int off = 32; off > 0; off >>= 1) sq += __shfl_down(sq, off, 64);
        if ((tid & 63) == 0) red[tid >> 6] = sq;
        __syncthreads();
        if (tid == 0) {
            double t = red[0];
            for (int w = 1; w < SG_WAVES; ++w) t += red[w];
            const double e = sqrt(t);
            s_err = e;
            s_verdict = (e < A.stop_thr) ? 1 : (!(fabs(e) < INFINITY) ? 2 : 0);
        }
        __syncthreads();
        err = s_err;
        done = s_verdict;
        if (done) break;
        have_vn = true;
    }
    for (int e = tid; e < n; e += SG_WG) A.U[at + e] = u[e], A.V[at + e] = v[e];
    if (tid == 0) {
        st->iters = ii;
        st->done = done;
        st->err = err;
    }
}

// plans[c][i][j] = exp(Ry[yi,yj] + Rx[xi,xj] + u_c[i] + v_c[j]) and the log-scalings to the caller's arrays
__global__ __launch_bounds__(256) void k_sg_plan(int H, int W, int64_t B, const double *__restrict__ Cy,
                                                 const double *__restrict__ Cx, double reg, const double *__restrict__ U,
                                                 const double *__restrict__ V, double *__restrict__ plans,
                                                 double *__restrict__ logu_out, double *__restrict__ logv_out) {
    const int n = H * W, nn = n * n;
    const int64_t step = static_cast<int64_t>(gridDim.x) * 256, e0 = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (plans)
        for (int64_t e = e0; e < B * nn; e += step) {
            const int64_t c = e / nn;
            const int r = static_cast<int>(e - c * nn), i = r / n, j = r - i * n;
            const int yi = i / W, xi = i - yi * W, yj = j / W, xj = j - yj * W;
            plans[e] = exp(Cy[yi * H + yj] / (-reg) + Cx[xi * W + xj] / (-reg) + U[c * n + i] + V[c * n + j]);
        }
    for (int64_t e = e0; e < B * n; e += step) {
        if (logu_out) logu_out[e] = U[e];
        if (logv_out) logv_out[e] = V[e];
    }
}

// lanes per output (log2) for LSEs of `len` terms over n outputs: doubled while a stage has fewer than 24 waves of work
// and every lane still gets a term, 4 lanes at most (the rule fitted in the header: 12 x 12 -> 4, 28 x 28 -> 2, 56 x 56 -> 1)
int sg_lanes(int64_t n, int64_t len) {
#ifdef SG_FORCE_LANES // experiments: make EXTRA=-DSG_FORCE_LANES=<log2 P, 0..3>
    return SG_FORCE_LANES;
#endif
    int lp = 0;
    while (lp < 2 && (int64_t{2} << lp) <= len && ((n << lp) + 63) / 64 < 24) ++lp;
    return lp;
}

} // namespace

SX_API int sx_sinkhorn_grid_dev(sx_ctx *ctx, int64_t H, int64_t W, int64_t B, const double *a, const double *b,
                                const double *Cy, const double *Cx, double reg, int64_t max_iter, double stop_thr,
                                double *plans, double *logu_out, double *logv_out, sx_sinkhorn_result *results) {
    SX_ENTER(ctx);
    SX_REQUIRE(H > 0 && W > 0, "H and W must be positive");
    SX_REQUIRE(B >= 1 && B <= INT32_MAX, "B must be at least 1");
    SX_REQUIRE(a && b && Cy && Cx && results, "NULL argument");
    SX_REQUIRE(reg > 0 && max_iter >= 0, "reg must be positive and max_iter non-negative");
    if (H > SG_CAP || W > SG_CAP || sg_need(H, W) > SG_CAP) {
        sx_set_error("grid %lld x %lld does not fit one CU's LDS: W*(W|1) + H*(H|1) + 4*H*W must be <= %d doubles",
                     static_cast<long long>(H), static_cast<long long>(W), SG_CAP);
        return SX_ERR_UNSUPPORTED;
    }
    hipStream_t s = ctx->stream;
    const size_t n = static_cast<size_t>(H * W), uB = static_cast<size_t>(B);
    const size_t st_bytes = (sizeof(SgState) * uB + 255) & ~static_cast<size_t>(255);
    SX_TRY(sx_reserve2(ctx, st_bytes + sizeof(double) * 4 * uB * n)); // states | log a | log b | U | V
    SgArgs A;
    A.H = static_cast<int>(H), A.W = static_cast<int>(W);
    A.lpx = sg_lanes(H * W, W), A.lpy = sg_lanes(H * W, H);
    A.a = a, A.b = b, A.Cy = Cy, A.Cx = Cx, A.reg = reg, A.stop_thr = stop_thr;
    A.st = static_cast<SgState *>(ctx->ws2);
    A.loga = reinterpret_cast<double *>(static_cast<char *>(ctx->ws2) + st_bytes);
    A.logb = A.loga + uB * n, A.U = A.logb + uB * n, A.V = A.U + uB * n;
    std::vector<SgState> host(uB);
    int64_t launched = 0;
    bool first = true, all_done = false;
    while (first || (launched < max_iter && !all_done)) { // max_iter = 0 still needs the start written
        for (int q = 0; q < SG_SYNC_LAUNCHES && (first || launched < max_iter); ++q) {
            A.it0 = launched;
            A.it1 = (launched + SG_LAUNCH_ITERS < max_iter) ? launched + SG_LAUNCH_ITERS : max_iter;
            A.first = first ? 1 : 0;
            hipLaunchKernelGGL(k_sg_solve, dim3(static_cast<unsigned>(B)), dim3(SG_WG), 0, s, A);
            launched = A.it1;
            first = false;
        }
        SX_HIP(hipGetLastError());
        SX_HIP(hipMemcpyAsync(host.data(), A.st, sizeof(SgState) * uB, hipMemcpyDeviceToHost, s));
        SX_HIP(hipStreamSynchronize(s));
        all_done = true;
        for (const SgState &h : host) all_done = all_done && h.done != 0;
    }
    if (plans || logu_out || logv_out) {
        const int64_t work = plans ? B * static_cast<int64_t>(n * n) : B * static_cast<int64_t>(n);
        const int64_t blocks = (work + 255) / 256;
        hipLaunchKernelGGL(k_sg_plan, dim3(static_cast<unsigned>(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, A.H, A.W, B,
                           Cy, Cx, reg, A.U, A.V, plans, logu_out, logv_out);
        SX_HIP(hipGetLastError());
        SX_HIP(hipStreamSynchronize(s));
    }
    for (size_t c = 0; c < uB; ++c) {
        results[c].iters = host[c].iters;
        results[c].status = host[c].done; // 0 iteration limit, 1 converged, 2 tested err not finite
        results[c].err = host[c].err;
    }
    return SX_OK;
}
