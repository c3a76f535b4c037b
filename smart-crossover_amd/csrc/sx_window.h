// LDS operand window of the column walk (K1 score_columns, K10 price).
//
// Both kernels are bound by the L1<->L2 fabric, not by HBM, when the y[row] gathers miss the 32 KiB
// vector L1: every miss moves a 128-byte line for 8 useful bytes (profiles/r01: 59 M L2 requests per
// K1 launch against 11 M needed by the streamed arrays, i.e. ~18 TB/s of L2 traffic).  When the row
// indices of a tile cluster inside a window of SXL_CAP rows -- block-angular / staircase LPs, time-
// expanded networks -- a workgroup instead loads that window once with coalesced loads into LDS and
// serves the gathers from there; SXL_RUN neighbouring tiles share one window load because their
// windows overlap almost entirely.  Indices outside the window fall back to global memory, so the
// result is bit-identical to the plain walk whatever the matrix looks like.
#pragma once

#include "sx_segwalk.h"

#include <type_traits>

#ifndef SXL_CAP_V
#define SXL_CAP_V 4096
#endif
constexpr int SXL_CAP = SXL_CAP_V;   // window length in doubles (32 KiB of LDS)
constexpr int SXL_CHUNK = 1024; // staged entries per chunk of the windowed walk: 8 KiB of LDS, so that window + chunk
                                // = 40 KiB and FOUR workgroups share a CU (2048: three; K1 0.341 -> 0.312 ms at c5)

struct sx_stage_win {
    const double *__restrict__ vec;
    const double *win;
    int64_t wlo;
    __device__ __forceinline__ void operator()(double v, int32_t i, double (&o)[1]) const {
        const uint64_t d = static_cast<uint64_t>(static_cast<int64_t>(i) - wlo);
        const double yv = (d < static_cast<uint64_t>(SXL_CAP)) ? win[d] : vec[i];
        o[0] = v * yv;
    }
};

// all 256 lanes: win[k] = vec[min(wlo + k, bound - 1)], 16 independent coalesced loads per lane.
// The caller synchronises before the first gather.
__device__ __forceinline__ void sx_window_fill(double *win, const double *__restrict__ vec, int64_t wlo,
                                               int64_t bound) {
#pragma unroll
    for (int r = 0; r < SXL_CAP / SX_WG; ++r) {
        const int k = r * SX_WG + threadIdx.x;
        int64_t row = wlo + k;
        if (row > bound - 1) row = bound - 1;
        win[k] = vec[row];
    }
}

// One run of a windowed walk: tiles [run * RUN, +RUN) of `tiles` behind the window of the run's middle tile.  All lanes
// of the workgroup call it; `reuse`: the workgroup has walked a run before (a kernel with one run per workgroup spares
// the first barrier).  `epi` is the calling kernel's epilogue object: load(seg, valid) requests its operands of a segment
// as soon as the lane knows it (they fly under the walk), finish(seg, sum) completes a valid segment from its sum.  The
// sums start from +0.0 and are those of the plain walk: the window only changes where an operand is read from.
template <int RUN, class Epi>
__device__ __forceinline__ void sx_window_walk(const int64_t *__restrict__ tiles, int64_t ntiles, int64_t run,
                                               const int32_t *__restrict__ win_lo, const int64_t *__restrict__ ptr,
                                               const int32_t *__restrict__ idx, const double *__restrict__ val,
                                               const double *__restrict__ vec, int64_t bound,
                                               sx_walk_lds<1, SXL_CHUNK> &lds, double *win, const bool reuse,
                                               Epi &epi) {
    const int64_t t0 = run * RUN;
    const int64_t t1 = (t0 + RUN < ntiles) ? t0 + RUN : ntiles;
    const int64_t wlo = win_lo[(t0 + t1 - 1) >> 1];
    if (reuse) __syncthreads(); // the previous run's gathers are done with the window
    sx_window_fill(win, vec, wlo, bound);
    __syncthreads();
    for (int64_t t = t0; t < t1; ++t) {
        double acc[1];
        int64_t seg;
        bool valid;
        auto pre = [&](int64_t sg, bool ok) { epi.load(sg, ok); };
        sx_segwalk<1, SXL_CHUNK>(tiles, t, ptr, idx, val, sx_stage_win{vec, win, wlo}, lds, seg, valid, acc, pre);
        if (valid) epi.finish(seg, acc[0]);
    }
}

// Host side: launch(std::integral_constant<int, R>) for the first R of the list that `run` (tiles per window load,
// sx_window_run_csc) reaches, the last R of the list otherwise: the instantiations a windowed kernel is built for.
template <int R, int... REST, class Launch>
inline void sx_window_with_run(int run, const Launch &launch) {
    if constexpr (sizeof...(REST) == 0) launch(std::integral_constant<int, R>{});
    else if (run >= R) launch(std::integral_constant<int, R>{});
    else sx_window_with_run<REST...>(run, launch);
}
