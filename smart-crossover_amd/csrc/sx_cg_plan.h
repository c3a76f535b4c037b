// Host arithmetic of the projector CG (K4, sx_cg.hip): launch grids, the workspace layout, what the host decides from
// ||b|| and tol before the loop, and the result values taken from the downloaded state.  Plain C++: no HIP, no error
// text -- arguments in, results out; every piece states its contract.  The three drivers of sx_cg.hip (single device,
// sharded over ranks, inner CG of the free branch) own every device call and take all of this from here.
// tests/native/cg_plan_check.cpp runs this header under the host sanitizers.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace sx_cg_plan {

// shared with the kernels (sx_cg.hip takes them from here)
constexpr int WG = 256;    // lanes per workgroup (= SX_WG of the walks)
constexpr int GRID = 2048; // workgroups of a grid-stride walk at most = partials a walk leaves at most
constexpr int VEC_GRID = 1024; // workgroups (= partials) of a vector kernel at most

// Workgroups of a grid-stride walk over `ntiles` tiles: at most GRID; with the XCD-contiguous tile map on and at least
// 64 tiles a multiple of 8, rounded down (every XCD the same number of workgroups); never below 1.
inline int walk_grid(int64_t ntiles, bool xcd_map) {
    int64_t g = ntiles < GRID ? ntiles : GRID;
    if (xcd_map && ntiles >= 64) g &= ~static_cast<int64_t>(7);
    return static_cast<int>(g < 1 ? 1 : g);
}

// Workgroups of a vector kernel over `len` elements: grid-stride with ~4 elements per lane, 1 .. VEC_GRID.  The
// drivers size it for the longer of their vectors, which keeps small problems from launching mostly idle blocks.
inline int vector_grid(int64_t len) {
    const int64_t g = (len + 4 * WG - 1) / (4 * WG);
    return static_cast<int>(g < 1 ? 1 : (g > VEC_GRID ? VEC_GRID : g));
}

// Byte offsets of  state | ppq[GRID] | prr[GRID] | z r p q [m] | w atz [max(n, 1)]  from a 256-byte aligned base, and
// the bytes to reserve (256 spare at the end).  m >= 1.  The single-device driver comes here with n >= 1 only, the
// sharded one also with an empty column block (n = 0), whose w still holds the one zero its finish reads: for both
// `bytes` is what each computed for itself before, 256 + 16 GRID + 8 (4 m + 2 max(n, 1)) + 256.
struct Layout {
    size_t state, ppq, prr, z, r, p, q, w, atz, bytes;
};
inline Layout layout(int64_t m, int64_t n) {
    const size_t d = sizeof(double), um = static_cast<size_t>(m), un = static_cast<size_t>(n > 0 ? n : 1);
    Layout L;
    L.state = 0;
    L.ppq = 256;
    L.prr = L.ppq + d * GRID;
    L.z = L.prr + d * GRID;
    L.r = L.z + d * um;
    L.p = L.r + d * um;
    L.q = L.p + d * um;
    L.w = L.q + d * um;
    L.atz = L.w + d * un;
    L.bytes = L.atz + d * un + 256;
    return L;
}

// What the host decides once it knows ||b||, before the first iteration.  `done` goes into the device state (1: every
// kernel of the loop returns at once), `run`: enter the loop at all, `trivial`: the legacy immediate exit of the
// reference's pinned scipy, ||b|| <= tol -> x0 = 0 is the answer.  scipy also tests ||r|| < tol ||b|| before the first
// iteration, which with r = b holds exactly when tol > 1 (and ||b|| > tol, or it was trivial already).  The two rules
// differ in that case alone:
//   single device: not trivial; the loop is skipped, `done` stays 0 and the result reports converged = 0;
//   sharded:       reported as trivial and `done` is set, so the caller's loop never starts.
// Both are kept as they are: callers see the difference (converged, trivial_out), so merging them changes behaviour.
struct Start {
    bool trivial;
    bool run;
    int done;
};
inline Start start_single(double bnrm, double tol) {
    const bool trivial = !(bnrm > tol);
    return {trivial, !trivial && !(bnrm < tol * bnrm), trivial ? 1 : 0};
}
inline Start start_sharded(double bnrm, double tol) {
    const bool trivial = !(bnrm > tol) || (bnrm < tol * bnrm);
    return {trivial, !trivial, trivial ? 1 : 0};
}

// sx_cg_result from the state as downloaded after the loop: rho[iters & 1] is r.r of the last completed iteration (the
// slot alternates with the iteration's parity; rho[0] = b.b before the first).
inline double rel_residual(const double rho[2], long long iters, double bnrm) {
    return bnrm > 0 ? std::sqrt(rho[iters & 1]) / bnrm : 0.0;
}
// the trivial exit counts as converged although no kernel ever set the flag
inline int converged(bool trivial, int state_converged) { return trivial ? 1 : state_converged; }

} // namespace sx_cg_plan
