// Lane-major tile slabs of the column walk behind the LDS operand window (K1 score_columns, K10 price).
//
// The windowed walk (sx_window.h) reads the CSC entries with wide coalesced loads and then has to rebuild every
// column's stored-order sum through LDS: products parked in a 8 KiB buffer, two barriers per 1,024 entries, lane t
// reading its products back at a 64-byte stride.  All of that follows from the storage order alone.  This second copy
// of the entries stores lane t's q-th entry where lane t's own coalesced load finds it, so that the sum is formed in a
// register -- same products, same order, same roundings -- with no product buffer and no barrier inside a tile.
//
// The only LDS left is the window, which takes the freed space and more (SXN_CAP below).
//
// It uses the matrix' CSC tile table as it stands (so win_lo[tile] keeps its meaning).  The slab of a tile of `ncol`
// columns whose longest has `L` entries (rounded up to even) over W = ncol rounded up to even lanes is one block:
//     uint8  len[256]                 column lengths, 0 for lanes >= ncol
//     int32  idx[L / 2][W][2]         entry pair (2p, 2p + 1) of lane t: 8 bytes, consecutive lanes adjacent
//     double val[L / 2][W][2]         likewise, 16 bytes
// i.e. 256 + 12 L W bytes, at byte offset off[tile] of `slab` (16-byte aligned).  A slot q >= len[t] holds value 0.0 and
// a valid row index (the start of the tile's window), so that its gather is harmless; the kernels never ADD it (a
// padded +0.0 product would turn a -0.0 sum into +0.0).
//
// A matrix gets the copy when every tile has L <= SXN_MAX_LEN and the slots sum L W over all tiles is at most 9/8 of
// its entries: the copy then stays within 12.5 % of the entries' size and the per-lane loop short.  Built on the device
// the first time K1 or K10 wants it, kept by the matrix, freed with it.
#pragma once

#include "sx_window.h"

struct sx_ctx;
struct sx_matrix;

constexpr int SXN_MAX_LEN = 64; // longest column of a tile that still gets a slab
constexpr int SXN_HDR = 256;    // bytes of the length table at the head of a slab
// Rows of this walk's LDS window, from the run's win_lo on: 48 KiB, three workgroups per CU.  The 8 KiB the product
// buffer no longer takes go into the window and half a window more: what a gather that misses the window costs is the
// largest single item of these kernels (c5 staircase, one process, K1 / K10 in ms: no global gathers at all 0.260 / 0.182;
// 4,096 rows 0.327 / 0.255; 6,144 rows 0.304 / 0.252; 8,192 rows, two workgroups per CU, 0.305 / 0.290 --
// profiles/r07/lanes.md).
constexpr int SXN_CAP = 6144;
static_assert(SXN_CAP >= SXL_CAP && SXN_CAP % 2048 == 0, "the window table is built for SXL_CAP rows; the fill goes by 2,048");

struct sx_lanes {
    uint8_t *slab = nullptr; // device: all slabs, tile after tile
    int64_t *off = nullptr;  // device: ntiles + 1 byte offsets into slab
    int64_t ntiles = 0, slots = 0, bytes = 0;
};

// The lane-major copy of A's columns under ctx's "lanes" option: 1 built at the first request when the matrix is
// eligible; -1 (auto) the same from the second walk of the matrix on -- `walk`: the caller is K1 or K10 and not a query
// -- since a matrix that is scored once and dropped would pay 12 bytes per entry and a pass over them for one call; 0
// never.  *out = nullptr: none (not eligible, not due, switched off, no window table, or the stream is being captured
// before the first build).  Callers ask only where the windowed walk runs (sx_window_run_csc gave a run > 0).
int sx_lanes_get(sx_ctx *ctx, const sx_matrix *A, bool walk, const sx_lanes **out);
void sx_lanes_free(sx_lanes *S);

#ifdef __HIPCC__
typedef int sx_v2i __attribute__((ext_vector_type(2)));

// what the workgroup knows about a tile's slab (uniform)
struct sx_ln_tile {
    const uint8_t *base;
    int64_t seg0;
    int ncol, W, L;
};

__device__ __forceinline__ sx_ln_tile sx_ln_tile_at(const int64_t *__restrict__ tiles, const uint8_t *__restrict__ slab,
                                                    const int64_t *__restrict__ off, int64_t t) {
    sx_ln_tile g;
    g.seg0 = tiles[t];
    g.ncol = static_cast<int>(tiles[t + 1] - g.seg0);
    g.W = (g.ncol + 1) & ~1;
    const int64_t o = off[t];
    g.base = slab + o;
    g.L = static_cast<int>(static_cast<uint32_t>(off[t + 1] - o - SXN_HDR) / static_cast<uint32_t>(12 * g.W));
    return g;
}

// eight slots of a lane: entry pairs q0 / 2 .. q0 / 2 + 3
struct sx_ln_chunk {
    sx_v2i i[4];
    sx_v2d v[4];
};

// lanes past W and pairs past L / 2 load nothing: their slots read as (row `pad`, 0.0) and are never added.  The slab
// is read once per call and non-temporal, so that it does not displace the operand the gathers outside the window go
// for from L2 (c5 staircase, K1 0.343 -> 0.327 ms, K10 0.271 -> 0.255 with the 4,096-row window; the CSC stream of the
// staged walk never gained from it: profiles/r01/kbench_cache_policy.txt).
__device__ __forceinline__ void sx_ln_load(const sx_ln_tile &g, int q0, int32_t pad, sx_ln_chunk &c) {
    // (uniform plane address + the lane's 32-bit byte offset: one offset register serves all loads of a kind)
    const uint32_t t = threadIdx.x;
    const uint8_t *ip = g.base + SXN_HDR;
    const uint8_t *vp = ip + static_cast<size_t>(g.L) * g.W * 4;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        c.i[p] = sx_v2i{pad, pad};
        c.v[p] = sx_v2d{0.0, 0.0};
        const int pr = (q0 >> 1) + p;
        if (2 * pr < g.L && t < static_cast<uint32_t>(g.W)) {
            c.i[p] = __builtin_nontemporal_load(reinterpret_cast<const sx_v2i *>(ip + static_cast<size_t>(pr * g.W) * 8 + t * 8u));
            c.v[p] = __builtin_nontemporal_load(reinterpret_cast<const sx_v2d *>(vp + static_cast<size_t>(pr * g.W) * 16 + t * 16u));
        }
    }
}

// the operand of one slot: from the LDS window when the row lies inside it, from global memory otherwise
__device__ __forceinline__ double sx_ln_operand(const double *win, const double *__restrict__ vec, int32_t wlo, int32_t i) {
    const uint32_t d = static_cast<uint32_t>(i - wlo);
    const bool in = d < static_cast<uint32_t>(SXN_CAP);
    double y = win[in ? d : 0u];
    // (opaque to the optimiser: it would otherwise fold the two reads into ONE load through a generic pointer, the
    // FLAT load per entry of the staged walk, which takes the slow path to LDS and waits on both counters)
    asm("" : "+v"(y));
    if (!in) y = vec[i];
    return y;
}

// acc continued by the chunk's slots q0 .. q0 + 7 below len, left to right, each product rounded on its own
__device__ __forceinline__ void sx_ln_sum(const sx_ln_chunk &c, int q0, int len, const double *win,
                                          const double *__restrict__ vec, int32_t wlo, double &acc) {
    double y[8];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        y[2 * p] = sx_ln_operand(win, vec, wlo, c.i[p].x);
        y[2 * p + 1] = sx_ln_operand(win, vec, wlo, c.i[p].y);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const double p0 = c.v[p].x * y[2 * p], p1 = c.v[p].y * y[2 * p + 1];
        if (q0 + 2 * p < len) acc = acc + p0;
        if (q0 + 2 * p + 1 < len) acc = acc + p1;
    }
}

// One run of the lane-major walk: tiles [run * RUN, +RUN) behind a window that starts where sx_window_walk's does (the
// run's middle tile's win_lo) and is SXN_CAP rows long; same epilogue contract, same sums.  The first tile's loads are
// issued before the window fill, every later chunk's loads before the chunk in hand is summed.
template <int RUN, class Epi>
__device__ __forceinline__ void sx_lanes_walk(const int64_t *__restrict__ tiles, int64_t ntiles, int64_t run,
                                              const int32_t *__restrict__ win_lo, const uint8_t *__restrict__ slab,
                                              const int64_t *__restrict__ off, const double *__restrict__ vec,
                                              int64_t bound, double *win, const bool reuse, Epi &epi) {
    const int64_t t0 = run * RUN;
    const int64_t t1 = (t0 + RUN < ntiles) ? t0 + RUN : ntiles;
    const int32_t wlo = win_lo[(t0 + t1 - 1) >> 1];
    sx_ln_tile g = sx_ln_tile_at(tiles, slab, off, t0);
    int len = g.base[threadIdx.x];
    sx_ln_chunk cur;
    sx_ln_load(g, 0, wlo, cur);
    if (reuse) __syncthreads(); // the previous run's gathers are done with the window
    for (int h = 0; h < SXN_CAP / 2048; ++h) { // win[k] = vec[min(wlo + k, bound - 1)], eight loads per lane in flight
#pragma unroll
        for (int r = 0; r < 2048 / SX_WG; ++r) {
            const int k = h * 2048 + r * SX_WG + threadIdx.x;
            int64_t row = static_cast<int64_t>(wlo) + k;
            if (row > bound - 1) row = bound - 1;
            win[k] = vec[row];
        }
    }
    __syncthreads();
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t seg = g.seg0 + threadIdx.x;
        const bool valid = static_cast<int>(threadIdx.x) < g.ncol;
        epi.load(seg, valid);
        double acc = 0.0;
        const int L = g.L, mylen = len;
        int q0 = 0;
        do { // (a tile of empty columns has L = 0: one chunk of padding, nothing added)
            sx_ln_chunk nxt = cur; // (kept when this is the run's last chunk)
            const int q_here = q0;
            q0 += 8;
            if (q0 < L) {
                sx_ln_load(g, q0, wlo, nxt);
            } else if (t + 1 < t1) {
                g = sx_ln_tile_at(tiles, slab, off, t + 1);
                len = g.base[threadIdx.x];
                sx_ln_load(g, 0, wlo, nxt);
            }
            sx_ln_sum(cur, q_here, mylen, win, vec, wlo, acc);
            cur = nxt;
        } while (q0 < L);
        if (valid) epi.finish(seg, acc);
    }
}
#endif
