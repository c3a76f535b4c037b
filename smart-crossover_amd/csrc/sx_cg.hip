// K4: norm of the projection (I - Y^T (Y Y^T)^+ Y) v with Y = [A, I_<] diag(xx), v = diag(xx) c_std,
// by matrix-free conjugate gradients on the device (reference: get_projector_Xc / apply_projector /
// get_scale_factor, lp_methods/algorithms.py:162-193, which forms Y Y^T explicitly and calls
// scipy's cg with tol=1e-8, maxiter=1000).
//
// With xa = xx[:n] (structural columns) and xs = xx[n:] scattered to the '<' rows (0 elsewhere):
//     (Y Y^T) p = A (xa^2 .* (A^T p)) + xs^2 .* p          b = Y v = A (xa^2 .* c)
//     proj      = [ xa .* (c - A^T z) ;  -xs .* z ]         (slack costs are zero)
// One CG iteration is four launches: CSC pass (w), CSR pass (q, partial p.q), update of z and r
// (partial r.r), update of p.  Scalars live in device memory; every kernel returns at once when the
// `done` flag is set, so the host enqueues iterations in batches and polls the flag between batches.
// Reductions are two-stage with a fixed order: results are reproducible run to run.  The recurrence
// and the stopping rule (||r|| < tol*||b||, tested before each iteration; legacy immediate exit when
// ||b|| <= tol) are those of the reference's pinned scipy.
#include "sx_cg_plan.h"
#include "sx_graph.h"
#include "sx_internal.h"
#include "sx_rowblock.h"
#include "sx_segwalk.h"
#include "sx_window.h"

#include <cmath>

namespace {

namespace plan = sx_cg_plan;
constexpr int CG_CHUNK = 4096;       // entries per LDS chunk of the plain walks
constexpr int CG_GRID = plan::GRID;  // workgroups of the grid-stride SpMV passes = number of partials
static_assert(SX_WG == plan::WG, "the plan's grids assume the walks' workgroup");

struct CgState {
    double rho[2];     // r.r of the current / next iteration (indexed by iteration parity)
    double atol;       // tol * ||b||
    double sumsq;      // final ||proj||^2
    long long iters;   // completed iterations
    int done;          // 1: converged (or finished), kernels become no-ops
    int converged;
};

struct StageDot {
    const double *__restrict__ vec;
    __device__ __forceinline__ void operator()(double v, int32_t i, double (&o)[1]) const {
        o[0] = v * vec[i];
    }
};

// fixed-order block sum; result valid in thread 0
__device__ __forceinline__ double block_sum(double v) {
    __shared__ double s[SX_WG / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads(); // protect s[] against the previous use
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    return s[0] + s[1] + s[2] + s[3];
}

// every workgroup re-reduces the partial array in the same order -> identical value everywhere
__device__ __forceinline__ double reduce_partials(const double *__restrict__ partial, int np) {
    double v = 0.0;
    for (int k = threadIdx.x; k < np; k += SX_WG) v += partial[k];
    double tot = block_sum(v);
    __shared__ double bc;
    if (threadIdx.x == 0) bc = tot;
    __syncthreads();
    return bc;
}

// out[j] = scale[j]^2 * (A^T in)[j]                                     (CSC pass)
struct CgAtEpilogue { // load() requests the segment's operand before the walk streams its entries
    const double *__restrict__ scale;
    double *__restrict__ out;
    double s;
    __device__ __forceinline__ void load(int64_t seg, bool valid) { s = valid ? scale[seg] : 0.0; }
    __device__ __forceinline__ void finish(int64_t j, double sum) const { out[j] = (s * s) * sum; }
};

__global__ __launch_bounds__(SX_WG) void k_cg_at(const CgState *st, const int64_t *__restrict__ tiles,
                                                 int64_t ntiles, int swizzle,
                                                 const int64_t *__restrict__ colptr,
                                                 const int32_t *__restrict__ rowidx,
                                                 const double *__restrict__ val,
                                                 const double *__restrict__ in,
                                                 const double *__restrict__ scale,
                                                 double *__restrict__ out) {
    if (st->done) return;
    __shared__ sx_walk_lds<1, CG_CHUNK> lds;
    CgAtEpilogue epi{scale, out};
    int64_t t, t_end, t_step;
    sx_walk_range(ntiles, swizzle, t, t_end, t_step);
    for (; t < t_end; t += t_step) {
        double acc[1];
        int64_t j;
        bool valid;
        auto pre = [&](int64_t seg, bool ok) { epi.load(seg, ok); };
        sx_segwalk<1, CG_CHUNK>(tiles, t, colptr, rowidx, val, StageDot{in}, lds, j, valid, acc, pre);
        if (valid) epi.finish(j, acc[0]);
    }
}

// the same pass behind the LDS operand window (sx_window.h): grid-stride over runs of RUN tiles
template <int RUN>
__global__ __launch_bounds__(SX_WG) void k_cg_at_lw(const CgState *st, const int64_t *__restrict__ tiles,
                                                    int64_t ntiles, int swizzle, const int32_t *__restrict__ win_lo,
                                                    const int64_t *__restrict__ colptr,
                                                    const int32_t *__restrict__ rowidx,
                                                    const double *__restrict__ val, int64_t m,
                                                    const double *__restrict__ in,
                                                    const double *__restrict__ scale, double *__restrict__ out) {
    if (st->done) return;
    __shared__ sx_walk_lds<1, SXL_CHUNK> lds;
    __shared__ double win[SXL_CAP];
    CgAtEpilogue epi{scale, out};
    int64_t r, r_end, r_step;
    sx_walk_range((ntiles + RUN - 1) / RUN, swizzle, r, r_end, r_step);
    for (; r < r_end; r += r_step) sx_window_walk<RUN>(tiles, ntiles, r, win_lo, colptr, rowidx, val, in, m, lds, win, true, epi);
}

// q[i] = (A w)[i] + xs[i]^2 * p[i];  partial[block] = sum p[i]*q[i]       (CSR pass)
// with p == nullptr: q = A w only, partial = sum q[i]^2  (used for b = Y v and rho0 = b.b)
__global__ __launch_bounds__(SX_WG) void k_cg_a(const CgState *st, const int64_t *__restrict__ tiles,
                                                int64_t ntiles, int swizzle,
                                                const int64_t *__restrict__ rowptr,
                                                const int32_t *__restrict__ colidx,
                                                const double *__restrict__ val,
                                                const double *__restrict__ w,
                                                const double *__restrict__ xs,
                                                const double *__restrict__ p, double *__restrict__ q,
                                                double *__restrict__ partial) {
    if (st->done) return;
    __shared__ sx_walk_lds<1, CG_CHUNK> lds;
    int64_t t, t_end, t_step;
    sx_walk_range(ntiles, swizzle, t, t_end, t_step);
    double dot = 0.0;
    for (; t < t_end; t += t_step) {
        double acc[1];
        int64_t i;
        bool valid;
        double s = 0.0, pi = 0.0; // epilogue operands requested before the walk
        auto pre = [&](int64_t seg, bool ok) {
            if (ok && p) {
                s = xs[seg];
                pi = p[seg];
            }
        };
        sx_segwalk<1, CG_CHUNK>(tiles, t, rowptr, colidx, val, StageDot{w}, lds, i, valid, acc, pre);
        if (valid) {
            double qi = acc[0];
            if (p) {
                qi = qi + (s * s) * pi;
                dot += pi * qi;
            } else {
                dot += qi * qi;
            }
            q[i] = qi;
        }
    }
    const double tot = block_sum(dot);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// t[j] = xa[j]^2 * c[j]
__global__ __launch_bounds__(SX_WG) void k_cg_scale_c(int64_t n, const double *__restrict__ xa,
                                                      const double *__restrict__ c,
                                                      double *__restrict__ t) {
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; j < n;
         j += static_cast<int64_t>(gridDim.x) * SX_WG)
        t[j] = (xa[j] * xa[j]) * c[j];
}

// start: r = p = b (already in r), z = 0, rho[0] = sum(partial)
__global__ __launch_bounds__(SX_WG) void k_cg_init(CgState *st, int64_t m, const double *__restrict__ partial,
                                                   int np, const double *__restrict__ r,
                                                   double *__restrict__ p, double *__restrict__ z) {
    const double rho0 = reduce_partials(partial, np);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; i < m;
         i += static_cast<int64_t>(gridDim.x) * SX_WG) {
        p[i] = r[i];
        z[i] = 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->rho[0] = rho0;
        st->rho[1] = 0.0;
        st->iters = 0;
        st->done = 0;
        st->converged = 0;
        st->sumsq = 0.0;
        st->atol = 0.0; // set by the host once it knows ||b||
    }
}

// alpha = rho / (p.q);  z += alpha p;  r -= alpha q;  partial_rr[block] = sum r^2
__global__ __launch_bounds__(SX_WG) void k_cg_update_zr(const CgState *st, int parity, int64_t m,
                                                        const double *__restrict__ partial_pq, int np,
                                                        const double *__restrict__ p,
                                                        const double *__restrict__ q,
                                                        double *__restrict__ z, double *__restrict__ r,
                                                        double *__restrict__ partial_rr) {
    if (st->done) return;
    const double pq = reduce_partials(partial_pq, np);
    const double alpha = st->rho[parity] / pq;
    double acc = 0.0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; i < m;
         i += static_cast<int64_t>(gridDim.x) * SX_WG) {
        z[i] = z[i] + alpha * p[i];
        const double ri = r[i] - alpha * q[i];
        r[i] = ri;
        acc += ri * ri;
    }
    const double tot = block_sum(acc);
    if (threadIdx.x == 0) partial_rr[blockIdx.x] = tot;
}

// rho' = sum(partial_rr); stop test; beta = rho'/rho; p = r + beta p
__global__ __launch_bounds__(SX_WG) void k_cg_update_p(CgState *st, int parity, int64_t m,
                                                       const double *__restrict__ partial_rr, int np,
                                                       const double *__restrict__ r,
                                                       double *__restrict__ p) {
    if (st->done) return;
    const double rho_new = reduce_partials(partial_rr, np);
    const double rho_old = st->rho[parity];
    const bool stop = sqrt(rho_new) < st->atol;
    if (!stop) {
        const double beta = rho_new / rho_old;
        for (int64_t i = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; i < m;
             i += static_cast<int64_t>(gridDim.x) * SX_WG)
            p[i] = r[i] + beta * p[i]; // scipy: p *= beta; p += r  (same two roundings)
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->rho[parity ^ 1] = rho_new;
        st->iters = st->iters + 1;
        if (stop) {
            st->converged = 1;
            __threadfence();
            st->done = 1;
        }
    }
}

// partial[block] = sum_j (xa[j] * (c[j] - (A^T z)[j]))^2
__global__ __launch_bounds__(SX_WG) void k_cg_proj_cols(int64_t n, const double *__restrict__ xa,
                                                        const double *__restrict__ c,
                                                        const double *__restrict__ atz,
                                                        double *__restrict__ partial,
                                                        double *__restrict__ proj_out) {
    double acc = 0.0;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; j < n;
         j += static_cast<int64_t>(gridDim.x) * SX_WG) {
        const double pj = xa[j] * (c[j] - atz[j]);
        if (proj_out) proj_out[j] = pj;
        acc += pj * pj;
    }
    const double tot = block_sum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// r[i] += xs[i]^2 * cs[i];  partial = sum r[i]^2 (only when the slack columns carry a cost)
__global__ __launch_bounds__(SX_WG) void k_cg_slack_cost(int64_t m, const double *__restrict__ xs,
                                                         const double *__restrict__ cs, double *__restrict__ r,
                                                         double *__restrict__ partial) {
    double acc = 0.0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; i < m;
         i += static_cast<int64_t>(gridDim.x) * SX_WG) {
        const double s = xs[i];
        const double ri = r[i] + (s * s) * cs[i];
        r[i] = ri;
        acc += ri * ri;
    }
    const double tot = block_sum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ __launch_bounds__(SX_WG) void k_cg_proj_rows(int64_t m, const double *__restrict__ xs,
                                                        const double *__restrict__ cs,
                                                        const double *__restrict__ z,
                                                        double *__restrict__ partial,
                                                        double *__restrict__ proj_out) {
    double acc = 0.0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; i < m;
         i += static_cast<int64_t>(gridDim.x) * SX_WG) {
        // slack block of proj: xs .* (cs - z); without slack costs it is -xs .* z
        const double pi = cs ? xs[i] * (cs[i] - z[i]) : -(xs[i] * z[i]);
        if (proj_out) proj_out[i] = pi;
        acc += pi * pi;
    }
    const double tot = block_sum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ __launch_bounds__(SX_WG) void k_cg_finish(CgState *st, const double *__restrict__ pa, int na,
                                                     const double *__restrict__ pb, int nb) {
    const double a = reduce_partials(pa, na);
    const double b = reduce_partials(pb, nb);
    if (threadIdx.x == 0) st->sumsq = a + b;
}

__global__ void k_cg_set_atol(CgState *st, double atol, int done) {
    st->atol = atol;
    st->done = done;
}

__global__ void k_cg_ones(int64_t n, double *v) {
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; j < n;
         j += static_cast<int64_t>(gridDim.x) * SX_WG)
        v[j] = 1.0;
}

// out = scale^2 .* (A^T in) on gT workgroups: behind the LDS operand window when win_run (sx_window_run_csc) says so
void launch_cg_at(hipStream_t s, const CgState *st, const sx_matrix *A, int gT, int swzT, int win_run, const double *in,
                  const double *scale, double *out) {
    if (win_run >= 1)
        sx_window_with_run<4, 1>(win_run, [&](auto R) {
            hipLaunchKernelGGL(k_cg_at_lw<decltype(R)::value>, dim3(gT), dim3(SX_WG), 0, s, st, A->csc_tiles, A->n_csc_tiles,
                               swzT, A->csc_win_lo, A->csc_ptr, A->csc_idx, A->csc_val, A->m, in, scale, out);
        });
    else
        hipLaunchKernelGGL(k_cg_at, dim3(gT), dim3(SX_WG), 0, s, st, A->csc_tiles, A->n_csc_tiles, swzT, A->csc_ptr,
                           A->csc_idx, A->csc_val, in, scale, out);
}

// degenerate shapes: with no rows Y is empty and the projector is the identity, proj = xa .* c; with no
// columns the only directions are slack columns, which Y = diag(xs) pins to zero wherever xs != 0
__global__ __launch_bounds__(1024) void k_cg_no_rows(int64_t n, const double *__restrict__ xa,
                                                     const double *__restrict__ c, double *__restrict__ proj_cols,
                                                     double *__restrict__ sumsq_out) {
    __shared__ double part[16];
    double acc = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += 1024) {
        const double v = xa[j] * c[j];
        if (proj_cols) proj_cols[j] = v;
        acc = acc + v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = part[0];
        for (int w = 1; w < 16; ++w) t += part[w];
        *sumsq_out = t;
    }
}

// ------------------------------------------------------------------------------------------------------
// Host side.  The three drivers of this file -- single device, sharded over ranks, inner CG of the free branch -- are
// the stages below over a CgPlan (how the two passes over A are launched) and a CgBufs (where the vectors live); the
// arithmetic of both is sx_cg_plan.h's.  What differs between the drivers stands in the drivers.

struct CgPlan {
    const sx_matrix *A = nullptr;
    int gT = 1, gA = 1, gv = 1;      // workgroups of the column pass, of the plain row pass, of the vector kernels
    int swzT = 0, swzA = 0;          // XCD-contiguous tile map of the column / row pass
    int win_run = 0;                 // column pass behind the LDS operand window: tiles per load (0: plain walk)
    const sx_rowblock *rb = nullptr; // row pass over the column-blocked copy of the rows (nullptr: plain walk)
    int nA = 1;                      // partials the last row pass left in ppq
};

// vec_len: the longest vector of the vector kernels.  plain: the plain walks, and nothing is built for A -- the free
// branch's gathered block lives for one call.  Otherwise the window table and the row-block copy are built here on
// their first use, outside any graph capture; ws_bytes > 0 grows ctx->ws between the two, where the single-device
// driver always has.
int cg_plan(sx_ctx *ctx, const sx_matrix *A, int64_t vec_len, bool plain, size_t ws_bytes, CgPlan *pl) {
    pl->A = A;
    pl->swzT = sx_csc_swizzle(ctx, A);
    pl->swzA = sx_csr_swizzle(ctx, A);
    pl->gT = plan::walk_grid(A->n_csc_tiles, ctx->opt_xcd_swizzle != 0);
    pl->gA = pl->nA = plan::walk_grid(A->n_csr_tiles, ctx->opt_xcd_swizzle != 0);
    pl->gv = plan::vector_grid(vec_len);
    if (plain) return SX_OK;
    SX_TRY(sx_window_run_csc(ctx, A, &pl->win_run));
    if (ws_bytes) SX_TRY(sx_reserve(ctx, ws_bytes));
    return sx_rowblock_get(ctx, A, &pl->rb);
}

struct CgBufs {
    CgState *st = nullptr;
    double *ppq = nullptr, *prr = nullptr; // partials of p.q (or q.q) from the row pass, of r.r from the update
    double *z = nullptr, *r = nullptr, *p = nullptr, *q = nullptr; // [len]
    double *w = nullptr, *atz = nullptr;   // results of the column pass
    int64_t len = 0;
};

CgBufs cg_carve(void *base, int64_t m, int64_t n) {
    const plan::Layout L = plan::layout(m, n);
    char *at = static_cast<char *>(base);
    auto vec = [at](size_t off) { return reinterpret_cast<double *>(at + off); };
    CgBufs b;
    b.st = reinterpret_cast<CgState *>(at + L.state);
    b.ppq = vec(L.ppq), b.prr = vec(L.prr);
    b.z = vec(L.z), b.r = vec(L.r), b.p = vec(L.p), b.q = vec(L.q);
    b.w = vec(L.w), b.atz = vec(L.atz);
    b.len = m;
    return b;
}

// column pass: out = scale^2 .* (A^T in)
void cg_cols(sx_ctx *ctx, const CgPlan &pl, const CgBufs &b, const double *in, const double *scale, double *out) {
    launch_cg_at(ctx->stream, b.st, pl.A, pl.gT, pl.swzT, pl.win_run, in, scale, out);
}

// row pass: out = A vec, partials of out.out in ppq; with pvec the slack term is fused in, out = A vec + xs^2 .* pvec,
// partials of pvec.out.  pl.nA = number of partials either walk leaves
int cg_rows(sx_ctx *ctx, CgPlan &pl, const CgBufs &b, const double *vec, const double *xs, const double *pvec, double *out) {
    const sx_matrix *A = pl.A;
    if (pl.rb) return sx_rb_cg_a(ctx, pl.rb, A->n, b.st, vec, xs, pvec, out, b.ppq, CG_GRID, &pl.nA);
    hipLaunchKernelGGL(k_cg_a, dim3(pl.gA), dim3(SX_WG), 0, ctx->stream, b.st, A->csr_tiles, A->n_csr_tiles, pl.swzA,
                       A->csr_ptr, A->csr_idx, A->csr_val, vec, xs, pvec, out, b.ppq);
    pl.nA = pl.gA;
    return SX_OK;
}

// this device's share of b = Y v: out = A (xa^2 .* c)
int cg_rhs(sx_ctx *ctx, CgPlan &pl, const CgBufs &b, const double *xa, const double *xs, const double *c, double *out) {
    hipLaunchKernelGGL(k_cg_scale_c, dim3(pl.gv), dim3(SX_WG), 0, ctx->stream, pl.A->n, xa, c, b.w);
    return cg_rows(ctx, pl, b, b.w, xs, nullptr, out);
}

int cg_poll(sx_ctx *ctx, const CgBufs &b, CgState *host) {
    SX_HIP(hipMemcpyAsync(host, b.st, sizeof(*host), hipMemcpyDeviceToHost, ctx->stream));
    SX_HIP(hipStreamSynchronize(ctx->stream));
    return SX_OK;
}

void cg_arm(sx_ctx *ctx, const CgBufs &b, double atol, int done) {
    hipLaunchKernelGGL(k_cg_set_atol, dim3(1), dim3(1), 0, ctx->stream, b.st, atol, done);
}

// begin, with b in r and the n_rho0 partials of b.b in ppq: z = 0, p = r, rho0; ||b|| comes to the host, which decides
// by `rule` (sx_cg_plan.h) and arms the kernels with atol = tol ||b||
int cg_begin(sx_ctx *ctx, const CgPlan &pl, const CgBufs &b, int n_rho0, double tol, plan::Start (*rule)(double, double),
             double *bnrm, plan::Start *start) {
    hipLaunchKernelGGL(k_cg_init, dim3(pl.gv), dim3(SX_WG), 0, ctx->stream, b.st, b.len, b.ppq, n_rho0, b.r, b.p, b.z);
    CgState host;
    SX_TRY(cg_poll(ctx, b, &host));
    *bnrm = sqrt(host.rho[0]);
    *start = rule(*bnrm, tol);
    cg_arm(ctx, b, tol * *bnrm, start->done);
    return SX_OK;
}

// update, with q complete and the n_pq partials of p.q in ppq: alpha, z, r (n_rr partials of r.r in prr), stop test, beta, p
void cg_update(sx_ctx *ctx, const CgPlan &pl, const CgBufs &b, int parity, int n_pq, int n_rr) {
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_cg_update_zr, dim3(pl.gv), dim3(SX_WG), 0, s, b.st, parity, b.len, b.ppq, n_pq, b.p, b.q, b.z, b.r, b.prr);
    hipLaunchKernelGGL(k_cg_update_p, dim3(pl.gv), dim3(SX_WG), 0, s, b.st, parity, b.len, b.prr, n_rr, b.r, b.p);
}

// projection: columns xa .* (c - A^T z), gv partials of their squares in ppq; slack rows xs .* (cs - z), gv partials in
// prr.  A^T z is taken with unit scale (dividing xa^2 (A^T z) by xa would break on xa = 0), so w becomes a vector of
// ones first.  An empty column block (sharded only) leaves zeros in ppq.
int cg_project(sx_ctx *ctx, const CgPlan &pl, const CgBufs &b, const double *xa, const double *xs, const double *c,
               const double *cs, double atol, double *proj_cols, double *proj_rows) {
    hipStream_t s = ctx->stream;
    const int64_t n = pl.A->n;
    cg_arm(ctx, b, atol, 0); // re-arm the kernels
    if (n > 0) {
        hipLaunchKernelGGL(k_cg_ones, dim3(pl.gv), dim3(SX_WG), 0, s, n, b.w);
        cg_cols(ctx, pl, b, b.z, b.w, b.atz);
        hipLaunchKernelGGL(k_cg_proj_cols, dim3(pl.gv), dim3(SX_WG), 0, s, n, xa, c, b.atz, b.ppq, proj_cols);
    } else {
        SX_HIP(hipMemsetAsync(b.ppq, 0, sizeof(double) * pl.gv, s));
    }
    hipLaunchKernelGGL(k_cg_proj_rows, dim3(pl.gv), dim3(SX_WG), 0, s, b.len, xs, cs, b.z, b.prr, proj_rows);
    return SX_OK;
}

// what the loop left, from the state as downloaded after it (proj_norm is the caller's)
void cg_result(const CgState &host, double bnrm, bool trivial, sx_cg_result *result) {
    result->b_norm = bnrm;
    result->iters = host.iters;
    result->converged = plan::converged(trivial, host.converged);
    result->rel_residual = plan::rel_residual(host.rho, host.iters, bnrm);
}

} // namespace

SX_API int sx_projector_dev(sx_ctx *ctx, const sx_matrix *A, const double *xa, const double *xs,
                            const double *c, double tol, int maxiter, double *proj_cols,
                            double *proj_rows, sx_cg_result *result) {
    return sx_projector_std_dev(ctx, A, xa, xs, c, nullptr, tol, maxiter, proj_cols, proj_rows, result);
}

SX_API int sx_projector_std_dev(sx_ctx *ctx, const sx_matrix *A, const double *xa, const double *xs,
                                const double *c, const double *cs, double tol, int maxiter,
                                double *proj_cols, double *proj_rows, sx_cg_result *result) {
    SX_ENTER(ctx);
    SX_REQUIRE(A != nullptr && result != nullptr, "matrix or result is NULL");
    SX_REQUIRE(A->csr_ptr && A->csc_ptr, "the projector needs both layouts of A");
    SX_REQUIRE(xa && xs && c, "xa, xs or c is NULL");
    SX_REQUIRE(maxiter >= 0 && tol >= 0, "bad tol/maxiter");
    const int64_t m = A->m, n = A->n;
    memset(result, 0, sizeof(*result));
    if (m == 0 || n == 0) {
        // the reference's apply_projector on an empty Y returns v unchanged (algorithms.py:183-187)
        result->converged = 1;
        if (n == 0) {
            if (proj_rows && m > 0) SX_HIP(hipMemsetAsync(proj_rows, 0, sizeof(double) * static_cast<size_t>(m), ctx->stream));
            return SX_OK;
        }
        SX_TRY(sx_reserve(ctx, 256));
        double *sumsq = static_cast<double *>(ctx->ws);
        hipLaunchKernelGGL(k_cg_no_rows, dim3(1), dim3(1024), 0, ctx->stream, n, xa, c, proj_cols, sumsq);
        double host_sumsq = 0.0;
        SX_HIP(hipMemcpyAsync(&host_sumsq, sumsq, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        SX_HIP(hipStreamSynchronize(ctx->stream));
        result->proj_norm = sqrt(host_sumsq);
        return SX_OK;
    }

    // ---- plan: launch geometry, window table and row-block copy; the vectors in ctx->ws
    CgPlan pl;
    SX_TRY(cg_plan(ctx, A, m > n ? m : n, false, plan::layout(m, n).bytes, &pl));
    const CgBufs b = cg_carve(ctx->ws, m, n);
    hipStream_t s = ctx->stream;

    // ---- right-hand side b = A (xa^2 .* c) -> r, partials of b.b from the row pass
    SX_HIP(hipMemsetAsync(b.st, 0, sizeof(CgState), s));
    SX_TRY(cg_rhs(ctx, pl, b, xa, xs, c, b.r));
    int n_rho0 = pl.nA;
    if (cs) { // slack columns carry a cost: b += xs^2 .* cs, rho0 recomputed from the completed b
        hipLaunchKernelGGL(k_cg_slack_cost, dim3(pl.gv), dim3(SX_WG), 0, s, m, xs, cs, b.r, b.ppq);
        n_rho0 = pl.gv;
    }

    // ---- begin
    double bnrm = 0.0;
    plan::Start start;
    SX_TRY(cg_begin(ctx, pl, b, n_rho0, tol, plan::start_single, &bnrm, &start));

    // ---- loop
    CgState host;
    int launched = 0;
    bool finished = start.trivial;
    if (start.run) {
        auto enqueue_iteration = [&](int par) {
            cg_cols(ctx, pl, b, b.p, xa, b.w);
            (void)cg_rows(ctx, pl, b, b.w, xs, b.p, b.q); // no early return from inside a stream capture; the poll reports
            cg_update(ctx, pl, b, par, pl.nA, pl.gv);
        };
        // the loop is launch-bound on cache-resident problems (four ~4 us kernels per iteration): a
        // batch of 24 iterations (even, so the rho parity repeats) is captured once into a hipGraph and
        // replayed; the host polls the done flag between batches.  Direct launches serve the tail and
        // are the fallback when capture is unavailable.
        const int batch = 24;
        SxGraphBatch graph;
        if (maxiter >= 2 * batch && sx_graph_wanted(ctx, SX_GRAPH_HEED_NO_GRAPH_ENV)) {
            graph.capture(s, [&]() {
                for (int k = 0; k < batch; ++k) enqueue_iteration(k & 1);
            });
            (void)hipGetLastError();
        }
        while (launched < maxiter && !finished) {
            if (graph.ready() && launched + batch <= maxiter) {
                if (graph.launch(s) != hipSuccess) {
                    sx_set_error("hipGraphLaunch failed in the CG loop");
                    return SX_ERR_HIP;
                }
                launched += batch;
            } else {
                const int upto = (launched + batch < maxiter) ? launched + batch : maxiter;
                for (; launched < upto; ++launched) enqueue_iteration(launched & 1);
            }
            if (hipGetLastError() != hipSuccess || cg_poll(ctx, b, &host) != SX_OK) {
                sx_set_error("CG iteration batch failed");
                return SX_ERR_HIP;
            }
            finished = host.done != 0;
        }
    }
    SX_TRY(cg_poll(ctx, b, &host));
    cg_result(host, bnrm, start.trivial, result);

    // ---- projection and its norm: columns and slack rows in one sum
    SX_TRY(cg_project(ctx, pl, b, xa, xs, c, cs, tol * bnrm, proj_cols, proj_rows));
    hipLaunchKernelGGL(k_cg_finish, dim3(1), dim3(SX_WG), 0, s, b.st, b.ppq, pl.gv, b.prr, pl.gv);
    SX_HIP(hipGetLastError());
    SX_TRY(cg_poll(ctx, b, &host));
    result->proj_norm = sqrt(host.sumsq);
    return SX_OK;
}

SX_API int sx_projector_norm_dev(sx_ctx *ctx, const sx_matrix *A, const double *xa, const double *xs,
                                 const double *c, double tol, int maxiter, sx_cg_result *result) {
    return sx_projector_dev(ctx, A, xa, xs, c, tol, maxiter, nullptr, nullptr, result);
}

SX_API int sx_projector_norm(sx_ctx *ctx, const sx_matrix *A, const double *xa, const double *xs,
                             const double *c, double tol, int maxiter, sx_cg_result *result) {
    SX_ENTER(ctx);
    SX_REQUIRE(A != nullptr && result != nullptr, "matrix or result is NULL");
    SX_REQUIRE(xa && xs && c, "xa, xs or c is NULL");
    sx_stage st(ctx);
    void *dxa, *dxs, *dc;
    SX_TRY(st.in(xa, sizeof(double) * A->n, &dxa));
    SX_TRY(st.in(xs, sizeof(double) * A->m, &dxs));
    SX_TRY(st.in(c, sizeof(double) * A->n, &dc));
    return sx_projector_norm_dev(ctx, A, (double *)dxa, (double *)dxs, (double *)dc, tol, maxiter, result);
}

// ------------------------------------------------------------------------------------------------------
// The same CG with the columns of Y sharded over ranks (reference arithmetic
// lp_methods/algorithms.py:183-187).  A rank holds a column block A_loc (m x n_loc, both layouts) with its
// slice of xa and c; every m-vector (z, r, p, q, xs) is replicated and every rank performs the same vector
// updates, so the only exchange per iteration is ONE all-reduce(SUM) of the partial product q = A_loc w_loc --
// issued by the host between sx_cg_shard_local and sx_cg_shard_update on the stream the context runs on
// (torch.distributed: RCCL over xGMI); the dot products are then taken from replicated vectors and need no
// collective at all.  The slack block xs^2 .* p is added once, after the reduction.
namespace {

// q[i] += xs[i]^2 * p[i];  partial[block] = sum p[i]*q[i]
__global__ __launch_bounds__(SX_WG) void k_cg_add_slack(const CgState *st, int64_t m, const double *__restrict__ xs,
                                                        const double *__restrict__ p, double *__restrict__ q,
                                                        double *__restrict__ partial) {
    if (st->done) return;
    double acc = 0.0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; i < m;
         i += static_cast<int64_t>(gridDim.x) * SX_WG) {
        const double s = xs[i], pi = p[i];
        const double qi = q[i] + (s * s) * pi;
        q[i] = qi;
        acc += pi * qi;
    }
    const double tot = block_sum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// r = q (the reduced right-hand side), partial = sum r^2
__global__ __launch_bounds__(SX_WG) void k_cg_take_rhs(int64_t m, const double *__restrict__ q, double *__restrict__ r,
                                                       double *__restrict__ partial) {
    double acc = 0.0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; i < m;
         i += static_cast<int64_t>(gridDim.x) * SX_WG) {
        const double v = q[i];
        r[i] = v;
        acc += v * v;
    }
    const double tot = block_sum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

} // namespace

struct sx_cg_shard {
    sx_ctx *ctx = nullptr;
    const double *xa = nullptr, *xs = nullptr, *c = nullptr, *cs = nullptr; // the caller's, alive until close
    double tol = 0.0, bnrm = 0.0;
    char *block = nullptr; // one allocation, carved into b
    CgPlan pl;
    CgBufs b;
};

SX_API int sx_cg_shard_open(sx_ctx *ctx, const sx_matrix *A_loc, const double *xa_loc, const double *xs,
                            const double *c_loc, const double *cs, double tol, sx_cg_shard **out, double **reduce_vec) {
    SX_ENTER(ctx);
    SX_REQUIRE(A_loc && out && reduce_vec, "NULL argument");
    SX_REQUIRE(A_loc->csr_ptr && A_loc->csc_ptr, "the projector needs both layouts of the column block");
    SX_REQUIRE(xa_loc && xs && c_loc, "xa, xs or c is NULL");
    SX_REQUIRE(A_loc->m > 0 && tol >= 0, "empty row space or negative tolerance");
    sx_cg_shard *h = new (std::nothrow) sx_cg_shard();
    if (!h) {
        sx_set_error("out of host memory");
        return SX_ERR_NOMEM;
    }
    struct Guard { // a failure below must not leak the handle and its block
        sx_cg_shard *h;
        ~Guard() {
            if (h) {
                (void)sx_dfree(h->block);
                delete h;
            }
        }
    } guard{h};
    h->ctx = ctx;
    h->xa = xa_loc;
    h->xs = xs;
    h->c = c_loc;
    h->cs = cs;
    h->tol = tol;
    const int64_t m = A_loc->m, n = A_loc->n;
    SX_TRY(cg_plan(ctx, A_loc, m > n ? m : n, false, 0, &h->pl));
    const size_t bytes = plan::layout(m, n).bytes;
    if (sx_dmalloc(&h->block, bytes) != hipSuccess) {
        sx_set_error("hipMalloc of %zu bytes failed for the sharded projector", bytes);
        return SX_ERR_NOMEM;
    }
    h->b = cg_carve(h->block, m, n);
    hipStream_t s = ctx->stream;
    SX_HIP(hipMemsetAsync(h->b.st, 0, sizeof(CgState), s));
    // this rank's share of b = Y v -> q, to be summed over the ranks by the caller
    if (n > 0) SX_TRY(cg_rhs(ctx, h->pl, h->b, xa_loc, xs, c_loc, h->b.q));
    else SX_HIP(hipMemsetAsync(h->b.q, 0, sizeof(double) * static_cast<size_t>(m), s));
    SX_HIP(hipGetLastError());
    guard.h = nullptr;
    *out = h;
    *reduce_vec = h->b.q;
    return SX_OK;
}

SX_API int sx_cg_shard_start(sx_cg_shard *h, double *bnorm_out, int *trivial_out) {
    SX_REQUIRE(h != nullptr, "handle is NULL");
    sx_device_guard guard(h->ctx->device);
    hipStream_t s = h->ctx->stream;
    const CgBufs &b = h->b;
    const int gv = h->pl.gv;
    // the reduced right-hand side (against the single device's fused row pass): r = q, then the slack cost
    hipLaunchKernelGGL(k_cg_take_rhs, dim3(gv), dim3(SX_WG), 0, s, b.len, b.q, b.r, b.ppq);
    if (h->cs) hipLaunchKernelGGL(k_cg_slack_cost, dim3(gv), dim3(SX_WG), 0, s, b.len, h->xs, h->cs, b.r, b.ppq);
    plan::Start start;
    SX_TRY(cg_begin(h->ctx, h->pl, b, gv, h->tol, plan::start_sharded, &h->bnrm, &start));
    SX_HIP(hipGetLastError());
    if (bnorm_out) *bnorm_out = h->bnrm;
    if (trivial_out) *trivial_out = start.trivial ? 1 : 0;
    return SX_OK;
}

// w = xa^2 .* (A_loc^T p);  q = A_loc w   -- then the caller all-reduces q (the vector sx_cg_shard_open returned)
SX_API int sx_cg_shard_local(sx_cg_shard *h) {
    SX_REQUIRE(h != nullptr, "handle is NULL");
    sx_device_guard guard(h->ctx->device);
    if (h->pl.A->n > 0) {
        cg_cols(h->ctx, h->pl, h->b, h->b.p, h->xa, h->b.w);
        SX_TRY(cg_rows(h->ctx, h->pl, h->b, h->b.w, h->xs, nullptr, h->b.q));
    } else { // an empty block adds nothing to the sum; q still holds the last reduced vector
        SX_HIP(hipMemsetAsync(h->b.q, 0, sizeof(double) * static_cast<size_t>(h->b.len), h->ctx->stream));
    }
    SX_HIP(hipGetLastError());
    return SX_OK;
}

// with q reduced over the ranks: q += xs^2 .* p (against the single device's fused slack term), alpha, z, r, beta, p
// (iteration number = parity of rho's slot)
SX_API int sx_cg_shard_update(sx_cg_shard *h, int parity) {
    SX_REQUIRE(h != nullptr, "handle is NULL");
    sx_device_guard guard(h->ctx->device);
    const CgBufs &b = h->b;
    const int gv = h->pl.gv;
    hipLaunchKernelGGL(k_cg_add_slack, dim3(gv), dim3(SX_WG), 0, h->ctx->stream, b.st, b.len, h->xs, b.p, b.q, b.ppq);
    cg_update(h->ctx, h->pl, b, parity & 1, gv, gv);
    SX_HIP(hipGetLastError());
    return SX_OK;
}

SX_API int sx_cg_shard_poll(sx_cg_shard *h, int *done, int64_t *iters) {
    SX_REQUIRE(h != nullptr, "handle is NULL");
    sx_device_guard guard(h->ctx->device);
    CgState host;
    SX_TRY(cg_poll(h->ctx, h->b, &host));
    if (done) *done = host.done;
    if (iters) *iters = host.iters;
    return SX_OK;
}

// squared norms of this rank's part of the projection: its columns xa .* (c - A_loc^T z) (optionally written to
// proj_cols_loc) and the slack rows (identical on every rank: count them once); converged / iterations of the loop
SX_API int sx_cg_shard_finish(sx_cg_shard *h, double *proj_cols_loc, double *proj_rows, double *cols_sumsq,
                              double *rows_sumsq, sx_cg_result *result) {
    SX_REQUIRE(h != nullptr, "handle is NULL");
    sx_device_guard guard(h->ctx->device);
    sx_ctx *ctx = h->ctx;
    hipStream_t s = ctx->stream;
    const CgBufs &b = h->b;
    const int gv = h->pl.gv;
    CgState loop, host;
    SX_TRY(cg_poll(ctx, b, &loop));
    SX_TRY(cg_project(ctx, h->pl, b, h->xa, h->xs, h->c, h->cs, h->tol * h->bnrm, proj_cols_loc, proj_rows));
    // the two sums separately: k_cg_finish adds them, so run it once per term against a zeroed partner
    SX_HIP(hipMemsetAsync(b.w, 0, sizeof(double), s));
    hipLaunchKernelGGL(k_cg_finish, dim3(1), dim3(SX_WG), 0, s, b.st, b.ppq, gv, b.w, 1);
    SX_TRY(cg_poll(ctx, b, &host));
    const double cols = host.sumsq;
    hipLaunchKernelGGL(k_cg_finish, dim3(1), dim3(SX_WG), 0, s, b.st, b.prr, gv, b.w, 1);
    SX_TRY(cg_poll(ctx, b, &host));
    const double rows = host.sumsq;
    SX_HIP(hipGetLastError());
    if (cols_sumsq) *cols_sumsq = cols;
    if (rows_sumsq) *rows_sumsq = rows;
    if (result) {
        memset(result, 0, sizeof(*result));
        cg_result(loop, h->bnrm, false, result); // trivial went to the caller at start: converged is the loop's own flag
    }
    return SX_OK;
}

SX_API int sx_cg_shard_close(sx_cg_shard *h) {
    if (!h) return SX_OK;
    sx_device_guard guard(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    if (h->block) (void)sx_dfree(h->block);
    delete h;
    return SX_OK;
}

// ------------------------------------------------------------------------------------------------------
// Free-variable branch of get_projector_Xc (reference lp_methods/algorithms.py:173-180):
//     t = cg(A_2^T A_2, c_free, tol 1e-8, 1000 iterations);   c' = c_std[non-free] - A_1^T (A_2 t)
//     projection of X_1 c' onto {x : A_1 X_1 x + A_2 f = 0}        (a Gurobi QP in the reference)
// with A_2 the free columns and A_1 the other columns of the standard-form matrix [A, I_<].  Everything runs on
// the device: the normal equations of the free block by the same CG kernels with the two products swapped,
// the adjusted cost by one column pass (K1), and the QP as the limit of the ordinary projector in which the free
// columns carry a large scale tau and zero cost -- the penalty form, error O((||Y|| / (tau sigma_min(A_2)))^2);
// tau = 100 x the largest ordinary column scale, corrected for the ratio of column norms.  Parity with Gurobi's
// loose-tolerance answer is unpinned (no Gurobi); tests compare with the exact minimiser of the QP.
namespace {

__global__ __launch_bounds__(SX_WG) void k_free_flags(int64_t nf, const int64_t *__restrict__ free_idx,
                                                      uint8_t *__restrict__ is_free) {
    for (int64_t k = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; k < nf;
         k += static_cast<int64_t>(gridDim.x) * SX_WG)
        is_free[free_idx[k]] = 1;
}

// per column: squared norm; maxima as bit patterns of non-negative doubles: [0] all columns, [1] -(min over free
// columns) is awkward, so [1] holds the max of 1 / sqnorm over the free columns; [2] max xa over the non-free
__global__ __launch_bounds__(SX_WG) void k_free_column_stats(int64_t n, const int64_t *__restrict__ colptr,
                                                             const double *__restrict__ val,
                                                             const uint8_t *__restrict__ is_free,
                                                             const double *__restrict__ xa,
                                                             unsigned long long *__restrict__ stats) {
    double a = 0.0, b = 0.0, c = 0.0;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; j < n;
         j += static_cast<int64_t>(gridDim.x) * SX_WG) {
        double s = 0.0;
        for (int64_t e = colptr[j]; e < colptr[j + 1]; ++e) s += val[e] * val[e];
        a = fmax(a, s);
        if (is_free[j]) b = fmax(b, s > 0.0 ? 1.0 / s : INFINITY);
        else c = fmax(c, xa[j]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a = fmax(a, __shfl_down(a, o, 64));
        b = fmax(b, __shfl_down(b, o, 64));
        c = fmax(c, __shfl_down(c, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&stats[0], static_cast<unsigned long long>(__double_as_longlong(a)));
        atomicMax(&stats[1], static_cast<unsigned long long>(__double_as_longlong(b)));
        atomicMax(&stats[2], static_cast<unsigned long long>(__double_as_longlong(c)));
    }
}

__global__ __launch_bounds__(SX_WG) void k_free_max(int64_t m, const double *__restrict__ v, unsigned long long *slot) {
    double a = 0.0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; i < m;
         i += static_cast<int64_t>(gridDim.x) * SX_WG)
        a = fmax(a, v[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = fmax(a, __shfl_down(a, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(slot, static_cast<unsigned long long>(__double_as_longlong(a)));
}

// xa2 = xa with tau on the free columns; c_adj zeroed there
__global__ __launch_bounds__(SX_WG) void k_free_apply(int64_t n, const uint8_t *__restrict__ is_free, double tau,
                                                      const double *__restrict__ xa, double *__restrict__ xa2,
                                                      double *__restrict__ c_adj) {
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; j < n;
         j += static_cast<int64_t>(gridDim.x) * SX_WG) {
        const bool f = is_free[j] != 0;
        xa2[j] = f ? tau : xa[j];
        if (f) c_adj[j] = 0.0;
    }
}

// cs[i] = row '<' ? -g[i] : 0
__global__ __launch_bounds__(SX_WG) void k_free_slack_cost(int64_t m, const uint8_t *__restrict__ row_lt,
                                                           const double *__restrict__ g, double *__restrict__ cs) {
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; i < m;
         i += static_cast<int64_t>(gridDim.x) * SX_WG)
        cs[i] = row_lt[i] ? -g[i] : 0.0;
}

// partial sums of pc[j]^2 over non-free columns (mode 0) or pr[i]^2 over '<' rows (mode 1); masked-out entries are
// also zeroed in place so that the vectors handed back cover the QP's variables only
__global__ __launch_bounds__(SX_WG) void k_free_norm(int64_t n, const uint8_t *__restrict__ flag, int keep_when,
                                                     double *__restrict__ v, double *__restrict__ partial) {
    double acc = 0.0;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; j < n;
         j += static_cast<int64_t>(gridDim.x) * SX_WG) {
        if ((flag[j] != 0) == (keep_when != 0)) acc += v[j] * v[j];
        else v[j] = 0.0;
    }
    const double tot = block_sum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

inline double from_bits(unsigned long long b) {
    double d;
    memcpy(&d, &b, sizeof(d));
    return d;
}

} // namespace

SX_API int sx_projector_free_dev(sx_ctx *ctx, const sx_matrix *A, int64_t nf, const int64_t *free_idx, const double *xa,
                                 const double *xs, const double *c, const uint8_t *row_lt, double *proj_cols,
                                 double *proj_rows, sx_cg_result *result) {
    SX_ENTER(ctx);
    SX_REQUIRE(A && free_idx && xa && xs && c && row_lt && proj_cols && proj_rows && result, "NULL argument");
    SX_REQUIRE(A->csr_ptr && A->csc_ptr, "the projector needs both layouts of A");
    SX_REQUIRE(nf > 0 && nf <= A->n, "nf must be in 1 .. n");
    const int64_t m = A->m, n = A->n;
    hipStream_t s = ctx->stream;
    sx_stage tmp(ctx); // device temporaries, freed on return
    uint8_t *is_free;
    unsigned long long *stats;
    double *c_free, *c_adj, *xa2, *cs, *ones;
    unsigned char *st_block;
    CgBufs b; // of the inner CG on nf-vectors: z is t, q is A_2^T w; w (m) is A_2 p, later g = A_2 t; atz unused
    b.len = nf;
    SX_TRY(tmp.tmp(n, &is_free));
    SX_TRY(tmp.tmp(4, &stats));
    SX_TRY(tmp.tmp(nf, &c_free));
    SX_TRY(tmp.tmp(nf, &b.z));
    SX_TRY(tmp.tmp(nf, &b.r));
    SX_TRY(tmp.tmp(nf, &b.p));
    SX_TRY(tmp.tmp(nf, &b.q));
    SX_TRY(tmp.tmp(m, &b.w));
    SX_TRY(tmp.tmp(n, &c_adj));
    SX_TRY(tmp.tmp(n, &xa2));
    SX_TRY(tmp.tmp(m, &cs));
    SX_TRY(tmp.tmp(nf, &ones));
    SX_TRY(tmp.tmp(256, &st_block)); // the state, in a block of 256 bytes
    SX_TRY(tmp.tmp(CG_GRID, &b.ppq));
    SX_TRY(tmp.tmp(CG_GRID, &b.prr));
    b.st = reinterpret_cast<CgState *>(st_block);
    auto g1 = [](int64_t k) { return dim3(static_cast<unsigned>(plan::vector_grid(k))); };
    SX_HIP(hipMemsetAsync(is_free, 0, static_cast<size_t>(n), s));
    SX_HIP(hipMemsetAsync(stats, 0, 4 * sizeof(unsigned long long), s));
    SX_HIP(hipMemsetAsync(b.st, 0, sizeof(CgState), s));
    hipLaunchKernelGGL(k_free_flags, g1(nf), dim3(SX_WG), 0, s, nf, free_idx, is_free);

    // ---- t = cg(A_2^T A_2, c_free): the CG kernels with the row pass first (w = A_2 p, alpha = rho / (w.w))
    sx_matrix *A2 = nullptr;
    SX_TRY(sx_gather_columns_dev(ctx, A, free_idx, nf, &A2));
    struct Guard {
        sx_matrix *M;
        ~Guard() { (void)sx_matrix_destroy(M); }
    } guard{A2};
    SX_TRY(sx_gather_f64_dev(ctx, nf, free_idx, c, c_free));
    CgPlan pl; // plain walks: nothing is built for a block that lives for this call
    SX_TRY(cg_plan(ctx, A2, nf, true, 0, &pl));
    hipLaunchKernelGGL(k_cg_ones, dim3(pl.gv), dim3(SX_WG), 0, s, nf, ones);
    hipLaunchKernelGGL(k_cg_take_rhs, dim3(pl.gv), dim3(SX_WG), 0, s, nf, c_free, b.r, b.ppq); // r = c_free, partials r.r
    double bn = 0.0;
    plan::Start start;
    SX_TRY(cg_begin(ctx, pl, b, pl.gv, 1e-8, plan::start_single, &bn, &start));
    CgState host;
    for (int it = 0; start.run && it < 1000; ++it) {
        SX_TRY(cg_rows(ctx, pl, b, b.p, nullptr, nullptr, b.w)); // w = A_2 p, partials w.w
        cg_cols(ctx, pl, b, b.w, ones, b.q);                     // q = A_2^T w
        cg_update(ctx, pl, b, it & 1, pl.nA, pl.gv);
        if ((it % 25) == 24) {
            SX_TRY(cg_poll(ctx, b, &host));
            if (host.done) break;
        }
    }
    // ---- g = A_2 t (m-vector), adjusted cost c - A^T g on the structurals (zero on the free ones), -g on the slacks
    cg_arm(ctx, b, 0.0, 0); // re-arm
    SX_TRY(cg_rows(ctx, pl, b, b.z, nullptr, nullptr, b.w));
    SX_TRY(sx_score_columns_dev(ctx, A, b.w, c, nullptr, nullptr, nullptr, 0.0, c_adj, nullptr));
    hipLaunchKernelGGL(k_free_slack_cost, g1(m), dim3(SX_WG), 0, s, m, row_lt, b.w, cs);
    // ---- scale of the free columns
    hipLaunchKernelGGL(k_free_column_stats, g1(n), dim3(SX_WG), 0, s, n, A->csc_ptr, A->csc_val, is_free, xa, stats);
    hipLaunchKernelGGL(k_free_max, g1(m), dim3(SX_WG), 0, s, m, xs, stats + 3);
    unsigned long long hs[4];
    SX_HIP(hipMemcpyAsync(hs, stats, sizeof(hs), hipMemcpyDeviceToHost, s));
    SX_HIP(hipStreamSynchronize(s));
    const double norm_max = sqrt(from_bits(hs[0]));
    const double inv_min_free = from_bits(hs[1]); // max of 1 / ||a_j||^2 over the free columns
    const double norm_min_free = (inv_min_free > 0 && inv_min_free < INFINITY) ? sqrt(1.0 / inv_min_free) : 0.0;
    const double scale_max = fmax(from_bits(hs[2]), from_bits(hs[3]));
    const double ratio = norm_min_free > 0 ? norm_max / norm_min_free : 1.0;
    const double tau = 100.0 * fmax(scale_max, 1e-300) * fmax(1.0, ratio);
    hipLaunchKernelGGL(k_free_apply, g1(n), dim3(SX_WG), 0, s, n, is_free, tau, xa, xa2, c_adj);
    // ---- the penalised projector, then the norm over the QP's own variables (non-free columns, '<' rows)
    SX_TRY(sx_projector_std_dev(ctx, A, xa2, xs, c_adj, cs, 1e-8, 1000, proj_cols, proj_rows, result));
    const dim3 gn = g1(n), gm = g1(m);
    hipLaunchKernelGGL(k_free_norm, gn, dim3(SX_WG), 0, s, n, is_free, 0, proj_cols, b.ppq);
    hipLaunchKernelGGL(k_free_norm, gm, dim3(SX_WG), 0, s, m, row_lt, 1, proj_rows, b.prr);
    hipLaunchKernelGGL(k_cg_finish, dim3(1), dim3(SX_WG), 0, s, b.st, b.ppq, static_cast<int>(gn.x), b.prr, static_cast<int>(gm.x));
    SX_TRY(cg_poll(ctx, b, &host));
    SX_HIP(hipGetLastError());
    result->proj_norm = sqrt(host.sumsq);
    return SX_OK;
}
