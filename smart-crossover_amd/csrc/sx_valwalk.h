// Values-only sequential segment walk: sx_segwalk (sx_segwalk.h) for a sum that needs no gathered
// operand -- the per-column sum of squares of sx_norms.hip.  Same tiles, same chunks, same
// stage / consume split, same strictly left-to-right running sum per lane; but the inner index
// array is never read, so the walk streams 8 bytes per entry where the scoring walks stream 12.
//   stage   : every lane reads four entries with two 16-byte loads, applies `stage` to each (one
//             rounded operation per entry: the square) and parks the results in LDS;
//   consume : lane t adds the staged values of segment s0+t, in stored order, to its running sum.
// Compile with -ffp-contract=off.
#pragma once

#include "sx_segwalk.h"

// `pre(seg, valid)` as in sx_segwalk: the place to issue the loads of the epilogue's operands.
// On return acc holds the running sum of segment `seg` (valid lanes only), started from +0.0.
template <int CHUNK, class Stage, class Pre = sx_no_prologue>
__device__ __forceinline__ void sx_valwalk(const int64_t *__restrict__ tiles, int64_t tile,
                                           const int64_t *__restrict__ ptr, const double *__restrict__ val,
                                           const Stage &stage, sx_walk_lds<1, CHUNK> &lds, int64_t &seg,
                                           bool &valid, double &acc, const Pre &pre = Pre()) {
    const int tid = threadIdx.x;
    const sx_lane L = sx_walk_lane(tiles, tile, ptr, pre);
    seg = L.seg;
    valid = L.valid;
    const int64_t p_hi = L.p_hi;
    double sum[1] = {0.0};

    // two doubles per load: the stream starts on an even entry, so that every load is 16-byte aligned
    for (int64_t base = L.p_lo & ~static_cast<int64_t>(1); base < p_hi; base += CHUNK) {
        const double *__restrict__ src = val + base;
#pragma unroll
        for (int r = 0; r < CHUNK / SX_SWEEP; ++r) {
            const int64_t sweep0 = base + static_cast<int64_t>(r) * SX_SWEEP;
            if (sweep0 < p_hi) { // uniform across the workgroup
                const int off = r * SX_SWEEP + tid * 4;
                // lanes past the slice re-read its first quad (cached) instead of branching; their LDS
                // slots are never consumed.  A quad that begins inside the slice ends at most three
                // entries past it, inside the SX_PAD entries every value array is allocated with.
                const int eo = (base + off < p_hi) ? off : 0;
                const sx_v2d v01 = *reinterpret_cast<const sx_v2d *>(src + eo);
                const sx_v2d v23 = *reinterpret_cast<const sx_v2d *>(src + eo + 2);
                double2 *dst = reinterpret_cast<double2 *>(&lds.v[0][off]);
                dst[0] = make_double2(stage(v01.x), stage(v01.y));
                dst[1] = make_double2(stage(v23.x), stage(v23.y));
            }
        }
        __syncthreads();
        sx_consume(lds, L, base, sum);
        __syncthreads();
    }
    acc = sum[0];
}
