// Column norms and the norm-scaled column indicator |x_j| / ||A_j|| (gfx950).  An optional extra: the
// reference has no such score, nothing in the package selects it by default.
// See include/sxhip.h for the arithmetic contract.  Built with -ffp-contract=off: every square and
// every sum below is a separately rounded binary64 operation.
#include "sx_internal.h"
#include "sx_valwalk.h"

#include <cmath>

namespace {

constexpr int NORM_CHUNK = 4096; // staged entries per chunk: 32 KB of LDS

struct StageSquare {
    __device__ __forceinline__ double operator()(double v) const { return v * v; }
};

__device__ __forceinline__ double np_minimum(double a, double b) {
    return (a < b || a != a) ? a : b; // numpy.minimum: NaN wins
}

__device__ __forceinline__ double norm_numerator(int numerator, double xj, double lj, double uj) {
    if (numerator == SX_NORM_ABS) return fabs(xj);
    const bool is_free = (lj == -INFINITY) && (uj == INFINITY);
    const double gap = np_minimum(xj - lj, uj - xj);
    return is_free ? fabs(xj) : gap;
}

// an empty or all-zero column can never be basic: it scores +0.0 whatever x is
__device__ __forceinline__ double norm_score(double num, double q, double nrm) {
    return (q == 0.0) ? 0.0 : num / nrm;
}

// One workgroup per column tile: sum of squares by the values-only walk, then sqrt, numerator and division.
// x == nullptr: norms only.
__global__ __launch_bounds__(SX_WG) void k_column_norms(
    const int64_t *__restrict__ tiles, int64_t ntiles, int swizzle, const int64_t *__restrict__ colptr,
    const double *__restrict__ val, const double *__restrict__ x, const double *__restrict__ l,
    const double *__restrict__ u, int numerator, double *__restrict__ sumsq, double *__restrict__ norm,
    double *__restrict__ score) {
    __shared__ sx_walk_lds<1, NORM_CHUNK> lds;
    const int64_t tile = sx_tile_of_block(blockIdx.x, ntiles, swizzle);
    if (tile >= ntiles) return;
    double q = 0.0;
    int64_t j;
    bool valid;
    // the epilogue's operands are requested before the walk so their latency hides under it
    double xj = 0.0, lj = 0.0, uj = 0.0;
    auto pre = [&](int64_t seg, bool ok) {
        if (ok && x) {
            xj = x[seg];
            if (numerator != SX_NORM_ABS) {
                lj = l[seg];
                uj = u[seg];
            }
        }
    };
    sx_valwalk<NORM_CHUNK>(tiles, tile, colptr, val, StageSquare{}, lds, j, valid, q, pre);
    if (!valid) return;
    const double nrm = sqrt(q);
    if (sumsq) sumsq[j] = q;
    if (norm) norm[j] = nrm;
    if (score) score[j] = norm_score(norm_numerator(numerator, xj, lj, uj), q, nrm);
}

// The indicator from norms that are already there (they depend on A only): elementwise.
__global__ __launch_bounds__(SX_WG) void k_score_norm_ew(int64_t n, const double *__restrict__ x,
                                                         const double *__restrict__ l,
                                                         const double *__restrict__ u, int numerator,
                                                         const double *__restrict__ norm_in,
                                                         double *__restrict__ score) {
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * SX_WG + threadIdx.x; j < n;
         j += static_cast<int64_t>(gridDim.x) * SX_WG) {
        double lj = 0.0, uj = 0.0;
        if (numerator != SX_NORM_ABS) {
            lj = l[j];
            uj = u[j];
        }
        const double nrm = norm_in[j];
        // sqrt is monotone and sqrt(q) == 0 only for q == 0 (the smallest subnormal has a normal root)
        score[j] = norm_score(norm_numerator(numerator, x[j], lj, uj), nrm, nrm);
    }
}

int check_matrix(const sx_ctx *ctx, const sx_matrix *A) {
    SX_REQUIRE(A != nullptr, "matrix is NULL");
    SX_REQUIRE(A->ctx->device == ctx->device, "matrix lives on another device");
    SX_REQUIRE(A->csc_ptr != nullptr, "matrix has no CSC layout (row shard?)");
    return SX_OK;
}

int launch_walk(sx_ctx *ctx, const sx_matrix *A, const double *x, const double *l, const double *u, int numerator,
                double *sumsq, double *norm, double *score) {
    const int swz = (ctx->opt_xcd_swizzle && A->n_csc_tiles >= 64) ? 1 : 0;
    const unsigned grid = sx_xcd_grid(A->n_csc_tiles, swz);
    hipLaunchKernelGGL(k_column_norms, dim3(grid), dim3(SX_WG), 0, ctx->stream, A->csc_tiles, A->n_csc_tiles, swz,
                       A->csc_ptr, A->csc_val, x, l, u, numerator, sumsq, norm, score);
    SX_HIP(hipGetLastError());
    return SX_OK;
}

} // namespace

SX_API int sx_column_norms_dev(sx_ctx *ctx, const sx_matrix *A, double *sumsq, double *norm) {
    SX_ENTER(ctx);
    SX_TRY(check_matrix(ctx, A));
    if (A->n == 0 || (!sumsq && !norm)) return SX_OK;
    return launch_walk(ctx, A, nullptr, nullptr, nullptr, SX_NORM_ABS, sumsq, norm, nullptr);
}

SX_API int sx_score_norm_dev(sx_ctx *ctx, const sx_matrix *A, const double *x, const double *l, const double *u,
                             int numerator, const double *norm_in, double *score) {
    SX_ENTER(ctx);
    SX_TRY(check_matrix(ctx, A));
    SX_REQUIRE(numerator == SX_NORM_ABS || numerator == SX_NORM_GAP, "unknown numerator %d", numerator);
    if (A->n == 0) return SX_OK;
    SX_REQUIRE(x && score, "x or score is NULL");
    SX_REQUIRE(numerator == SX_NORM_ABS || (l && u), "the gap numerator needs l and u");
    if (!norm_in) return launch_walk(ctx, A, x, l, u, numerator, nullptr, nullptr, score);
    int64_t nb = (A->n + SX_WG - 1) / SX_WG;
    if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(k_score_norm_ew, dim3(static_cast<unsigned>(nb)), dim3(SX_WG), 0, ctx->stream, A->n, x, l, u,
                       numerator, norm_in, score);
    SX_HIP(hipGetLastError());
    return SX_OK;
}

SX_API int sx_score_norm(sx_ctx *ctx, const sx_matrix *A, const double *x, const double *l, const double *u,
                         int numerator, const double *norm_in, double *score) {
    SX_ENTER(ctx);
    SX_TRY(check_matrix(ctx, A));
    SX_REQUIRE(numerator == SX_NORM_ABS || numerator == SX_NORM_GAP, "unknown numerator %d", numerator);
    if (A->n == 0) return SX_OK;
    SX_REQUIRE(x && score, "x or score is NULL");
    SX_REQUIRE(numerator == SX_NORM_ABS || (l && u), "the gap numerator needs l and u");
    const size_t nb = sizeof(double) * static_cast<size_t>(A->n);
    sx_stage st(ctx);
    void *dx, *dl = nullptr, *du = nullptr, *dn = nullptr, *ds;
    SX_TRY(st.in(x, nb, &dx));
    if (numerator != SX_NORM_ABS) {
        SX_TRY(st.in(l, nb, &dl));
        SX_TRY(st.in(u, nb, &du));
    }
    if (norm_in) SX_TRY(st.in(norm_in, nb, &dn));
    SX_TRY(st.in(nullptr, nb, &ds));
    SX_TRY(sx_score_norm_dev(ctx, A, (double *)dx, (double *)dl, (double *)du, numerator, (double *)dn, (double *)ds));
    SX_TRY(st.out(score, ds, nb));
    SX_HIP(hipStreamSynchronize(ctx->stream));
    return SX_OK;
}
