// Builder of the lane-major tile slabs (sx_lanes.h): one pass measures every tile and decides eligibility from a
// 16-byte record, a scan lays the slabs out, one pass copies the entries.  All on the device, once per matrix.
#include "sx_internal.h"
#include "sx_lanes.h"

namespace {

// per tile: bytes[t] of its slab (longest column clamped to SXN_MAX_LEN: only read when the matrix is eligible);
// rec[0] = longest column of the matrix, rec[1] = slots L W over all tiles
__global__ __launch_bounds__(SX_WG) void k_ln_measure(const int64_t *__restrict__ tiles, const int64_t *__restrict__ ptr,
                                                      int64_t *__restrict__ bytes, unsigned long long *__restrict__ rec) {
    __shared__ long long wmax[SX_WG / 64];
    const int64_t t = blockIdx.x;
    const int64_t s0 = tiles[t];
    const int ncol = static_cast<int>(tiles[t + 1] - s0);
    const int lane = threadIdx.x;
    long long len = (lane < ncol) ? ptr[s0 + lane + 1] - ptr[s0 + lane] : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long other = __shfl_down(len, o, 64);
        len = other > len ? other : len;
    }
    if ((lane & 63) == 0) wmax[lane >> 6] = len;
    __syncthreads();
    if (lane == 0) {
        for (int w = 1; w < SX_WG / 64; ++w) len = wmax[w] > len ? wmax[w] : len;
        const long long L = ((len < SXN_MAX_LEN ? len : SXN_MAX_LEN) + 1) & ~1LL;
        const long long W = (ncol + 1) & ~1;
        bytes[t] = SXN_HDR + 12 * L * W;
        atomicMax(&rec[0], static_cast<unsigned long long>(len));
        atomicAdd(&rec[1], static_cast<unsigned long long>(L * W));
    }
}

// lane t of tile `blockIdx.x` copies its column, pair by pair, and pads up to L with (pad row, 0.0)
__global__ __launch_bounds__(SX_WG) void k_ln_fill(const int64_t *__restrict__ tiles, const int64_t *__restrict__ ptr,
                                                   const int32_t *__restrict__ idx, const double *__restrict__ val,
                                                   const int32_t *__restrict__ win_lo, const int64_t *__restrict__ off,
                                                   uint8_t *__restrict__ slab) {
    const int64_t t = blockIdx.x;
    const sx_ln_tile g = sx_ln_tile_at(tiles, slab, off, t);
    uint8_t *base = slab + off[t];
    const int lane = threadIdx.x;
    int64_t cs = 0;
    int len = 0;
    if (lane < g.ncol) {
        cs = ptr[g.seg0 + lane];
        len = static_cast<int>(ptr[g.seg0 + lane + 1] - cs);
    }
    base[lane] = static_cast<uint8_t>(len);
    if (lane >= g.W) return;
    const int32_t pad = win_lo[t];
    sx_v2i *ip = reinterpret_cast<sx_v2i *>(base + SXN_HDR);
    sx_v2d *vp = reinterpret_cast<sx_v2d *>(base + SXN_HDR + static_cast<size_t>(g.L) * g.W * 4);
    for (int p = 0; 2 * p < g.L; ++p) {
        sx_v2i i2{pad, pad};
        sx_v2d v2{0.0, 0.0};
        if (2 * p < len) {
            i2.x = idx[cs + 2 * p];
            v2.x = val[cs + 2 * p];
        }
        if (2 * p + 1 < len) {
            i2.y = idx[cs + 2 * p + 1];
            v2.y = val[cs + 2 * p + 1];
        }
        ip[p * g.W + lane] = i2;
        vp[p * g.W + lane] = v2;
    }
}

} // namespace

void sx_lanes_free(sx_lanes *S) {
    if (!S) return;
    (void)sx_dfree(S->slab);
    (void)sx_dfree(S->off);
    delete S;
}

// measure, decide, lay out, copy; *out stays nullptr for a matrix that is not eligible
static int lanes_build(sx_ctx *ctx, const sx_matrix *A, sx_lanes **out) {
    *out = nullptr;
    const int64_t nt = A->n_csc_tiles;
    if (nt == 0 || A->nnz == 0) return SX_OK;
    sx_arena tmp(ctx);
    SX_TRY(tmp.own((sizeof(int64_t) * static_cast<size_t>(nt) + 255 + 256) & ~static_cast<size_t>(255)));
    int64_t *bytes = nullptr;
    unsigned long long *rec = nullptr, h[2] = {0, 0};
    SX_TRY(tmp.get(static_cast<size_t>(nt), &bytes));
    SX_TRY(tmp.get(2, &rec));
    SX_HIP(hipMemsetAsync(rec, 0, sizeof(h), ctx->stream));
    hipLaunchKernelGGL(k_ln_measure, dim3(static_cast<unsigned>(nt)), dim3(SX_WG), 0, ctx->stream, A->csc_tiles, A->csc_ptr,
                       bytes, rec);
    SX_HIP(hipGetLastError());
    SX_HIP(hipMemcpyAsync(h, rec, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    SX_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t slots = static_cast<int64_t>(h[1]);
    if (h[0] > static_cast<unsigned long long>(SXN_MAX_LEN) || 8 * slots > 9 * A->nnz) return SX_OK;
    sx_lanes *S = new (std::nothrow) sx_lanes;
    if (!S) {
        sx_set_error("out of host memory for the lane-major layout");
        return SX_ERR_NOMEM;
    }
    S->ntiles = nt;
    S->slots = slots;
    S->bytes = SXN_HDR * nt + 12 * slots;
    int rc = SX_OK;
    if (sx_dmalloc(&S->off, sizeof(int64_t) * static_cast<size_t>(nt + 1)) != hipSuccess ||
        sx_dmalloc(&S->slab, static_cast<size_t>(S->bytes)) != hipSuccess) {
        sx_set_error("out of device memory for the lane-major layout (%lld bytes)", static_cast<long long>(S->bytes));
        rc = SX_ERR_NOMEM;
    }
    if (rc == SX_OK) rc = sx_scan_exclusive(ctx, bytes, nt, S->off);
    if (rc == SX_OK) {
        hipLaunchKernelGGL(k_ln_fill, dim3(static_cast<unsigned>(nt)), dim3(SX_WG), 0, ctx->stream, A->csc_tiles, A->csc_ptr,
                           A->csc_idx, A->csc_val, A->csc_win_lo, S->off, S->slab);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
            sx_set_error("lane-major layout kernel failed");
            rc = SX_ERR_HIP;
        }
    }
    if (rc != SX_OK) {
        sx_lanes_free(S);
        return rc;
    }
    *out = S;
    return SX_OK;
}

int sx_lanes_get(sx_ctx *ctx, const sx_matrix *A, bool walk, const sx_lanes **out) {
    *out = nullptr;
    if (ctx->opt_lanes == 0 || !A->csc_win_lo) return SX_OK;
    if (!A->lanes_tried) {
        if (ctx->opt_lanes < 0 && !A->lanes_asked) { // auto: a matrix that is walked once does not pay for a copy
            if (walk) A->lanes_asked = 1;
            return SX_OK;
        }
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(ctx->stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
            (void)hipGetLastError();
            return SX_OK; // (no build under capture: this call takes the staged walk)
        }
        A->lanes_tried = 1;
        SX_TRY(lanes_build(ctx, A, &A->lanes));
    }
    *out = A->lanes;
    return SX_OK;
}

SX_API int sx_matrix_lanes_info(sx_ctx *ctx, const sx_matrix *A, int64_t *info /* [3] */) {
    SX_ENTER(ctx);
    SX_REQUIRE(A != nullptr && info != nullptr, "NULL argument");
    const sx_lanes *S = nullptr;
    int run = 0;
    SX_TRY(sx_window_run_csc(ctx, A, &run));
    if (run) SX_TRY(sx_lanes_get(ctx, A, false, &S));
    info[0] = S ? S->ntiles : 0;
    info[1] = S ? S->slots : 0;
    info[2] = S ? S->bytes : 0;
    return SX_OK;
}
