// Host arithmetic of the dense-inverse simplex driver (K16, sx_simplex.hip): sizes, intervals, launch geometry, the test
// "does the session's inverse belong to the basis handed in", and the map from how a phase stopped to a result status.
// Plain C++: no HIP, no error text, nothing captured -- arguments in, results out; every piece states its contract.
// The driver owns every device call.  tests/native/simplex_plan_check.cpp runs this header under the host sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace sx_spx_plan {

// shared with the kernels (sx_simplex.hip takes them from here)
constexpr int WG = 256;       // lanes per workgroup (= SX_WG of the walks)
constexpr int GRID = 1024;    // price workgroups (= partials) at most
constexpr int DEFER = 64;     // pivots whose inverse updates are held back and folded in together
constexpr int FOLD_COLS = 64; // columns of the inverse per workgroup of the scalar fold
constexpr int FM_KT = 64, FM_IC = 16; // matrix-core fold: column tiles x row chunks of one super-block of workgroups
constexpr int BASIC = 0;      // the reference's basis code of a basic variable / of a row whose logical is basic

// Pivots a solve may take when the caller names no limit (max_iter <= 0).
inline int64_t default_max_iter(int64_t m, int64_t n) { return 50 * (m + n) + 1000; }

// Device bytes of a solve with an inverse of its own: the dense m x m inverse, ~600 B per row, 40 B per variable
// (N = n + m).  The solve is taken when that is at most 0.9 of the HBM that is free now.
inline double inverse_bytes(int64_t m, int64_t N) {
    return 8.0 * static_cast<double>(m) * static_cast<double>(m) + 600.0 * static_cast<double>(m) + 40.0 * static_cast<double>(N);
}
inline bool inverse_fits(int64_t m, int64_t N, size_t free_bytes) {
    return !(inverse_bytes(m, N) > 0.9 * static_cast<double>(free_bytes));
}

// Bytes of the one block a solve carves its device arrays from: at least the sum of its requests, each rounded up to
// 256 bytes (simplex_plan_check.cpp replays the list).  35 B per variable (34 of the solve, 1 of the basis codes a
// re-inversion reads back: without it a wide LP, n > 7 m + 5,000 or so, sent its last requests to allocations of their own),
// 56 B per row, pricing partials for `grid` + m / 64 + 64 workgroups, 32 + 16 roundings; the inverse unless a session
// holds it; the pending updates of a batch with `defer`; ratio candidates and tickets; the Devex weights with `devex`.
inline size_t arena_bytes(int64_t m, int64_t N, bool has_session, bool defer, bool devex, int grid) {
    const size_t um = static_cast<size_t>(m), uN = static_cast<size_t>(N);
    size_t bytes = 35 * uN + 56 * um + 24 * (static_cast<size_t>(grid) + um / 64 + 64) + 32 * 256 + 4096;
    if (!has_session) bytes += sizeof(double) * um * um + 256;
    if (defer) bytes += 2 * sizeof(double) * um * DEFER + 1024;
    bytes += 32 * (um / WG + 2) + 1024;
    if (devex) bytes += sizeof(double) * uN + 256;
    return bytes;
}

// Pivots between two recomputations of x_B and y from scratch.  Those cost two passes over the m x m inverse, a pivot
// O(m): the interval grows with m so that the refresh stays a small share of the pivots between two of them --
// 64 (m / 2048)^2, rounded down to a multiple of 64 and clamped to 64 .. 2048 (64 up to m = 2048, 2048 from m = 11.6k on).
inline int64_t refresh_interval(int64_t m) {
    const double scale = static_cast<double>(m) / 2048.0;
    const double sq = 64.0 * scale * scale;
    if (!(sq < 4096.0)) return 2048; // (also keeps the conversion below in range)
    const int64_t want = (static_cast<int64_t>(sq) / 64) * 64;
    return want < 64 ? 64 : (want > 2048 ? 2048 : want);
}

// Scalar fold (k_spx_fold): one workgroup per WG rows x FOLD_COLS columns of the inverse, row blocks fastest.
inline int fold_col_tiles(int64_t m) { return static_cast<int>((m + FOLD_COLS - 1) / FOLD_COLS); }
inline unsigned fold_grid(int64_t m) { return static_cast<unsigned>(((m + WG - 1) / WG) * fold_col_tiles(m)); }
// Matrix-core fold (k_spx_fold_mfma): nkt column tiles of 16, nic row chunks of 256; the grid covers whole
// super-blocks of FM_KT x FM_IC workgroups (those past the matrix return at once).
inline int64_t fm_nkt(int64_t m) { return (m + 15) / 16; }
inline int64_t fm_nic(int64_t m) { return (m + 255) / 256; }
inline unsigned fm_grid(int64_t m) {
    return static_cast<unsigned>(((fm_nkt(m) + FM_KT - 1) / FM_KT) * ((fm_nic(m) + FM_IC - 1) / FM_IC) * FM_KT * FM_IC);
}

// Does a kept inverse belong to the basis being handed in?  head_ids: per basis position of the kept inverse the
// caller's stable id of a structural (>= 0) or -(r + 1) for the logical of row r.  vb[n], cb[m]: the warm basis in
// the reference's codes (BASIC = 0); col_ids[n]: the stable ids of this round's columns, which may have been permuted,
// dropped or added since the inverse was left.  True exactly when
//   - head_ids has m positions and the basis names m basic variables (structurals with vb = 0 plus rows with cb = 0),
//   - every structural id of the kept head is found among the basic columns, each basic column serving one position
//     (so a head that names an id twice, or two basic columns with one id, do not match),
//   - every logical -(r + 1) of the kept head has r < m and cb[r] = 0,
//   - no basic column is left over;
// head_new[i] is then the variable at position i in this round's numbering: column j, or n + r.  When false,
// head_new holds nothing of use.
inline bool match_kept_head(const std::vector<int64_t> &head_ids, const int8_t *vb, const int8_t *cb, const int64_t *col_ids,
                            int64_t n, int64_t m, std::vector<int32_t> &head_new) {
    head_new.assign(static_cast<size_t>(m > 0 ? m : 0), 0);
    if (m < 0 || static_cast<int64_t>(head_ids.size()) != m) return false;
    std::unordered_map<int64_t, int32_t> basic_of_id;
    int64_t n_basic = 0;
    for (int64_t j = 0; j < n; ++j)
        if (vb[j] == BASIC) {
            basic_of_id.emplace(col_ids[j], static_cast<int32_t>(j));
            ++n_basic;
        }
    for (int64_t i = 0; i < m; ++i) n_basic += (cb[i] == BASIC) ? 1 : 0;
    if (n_basic != m) return false;
    for (int64_t i = 0; i < m; ++i) {
        const int64_t id = head_ids[static_cast<size_t>(i)];
        if (id >= 0) {
            auto it = basic_of_id.find(id);
            if (it == basic_of_id.end()) return false;
            head_new[static_cast<size_t>(i)] = it->second;
            basic_of_id.erase(it); // every basic column serves one position
        } else {
            const int64_t r = -(id + 1);
            if (r >= m || cb[r] != BASIC) return false;
            head_new[static_cast<size_t>(i)] = static_cast<int32_t>(n + r);
        }
    }
    return basic_of_id.empty();
}

// The inverse of match_kept_head: the ids under which a basis head (variable per position, < n structural, else
// n + row) is remembered.  Without col_ids every structural gets id 0 (such a head is never marked valid).
inline void head_ids_of(const std::vector<int32_t> &head, const int64_t *col_ids, int64_t n, std::vector<int64_t> &out) {
    out.resize(head.size());
    for (size_t i = 0; i < head.size(); ++i) {
        const int32_t k = head[i];
        out[i] = (k < n) ? (col_ids ? col_ids[k] : 0) : -(static_cast<int64_t>(k - n) + 1);
    }
}

// status of sx_simplex_result; OPEN: not decided yet
enum : int { OPEN = -1, OPTIMAL = 0, INFEASIBLE = 1, UNBOUNDED = 2, ITER_LIMIT = 3, NUMERICAL = 4 };
// What a phase that stopped with SpxState::done = `done` (0 still running at the budget, 1 no candidate, 2 unbounded,
// 3 breakdown) decides on its own.  OPEN: it ran to the end for its costs, and the driver looks at the point.
inline int phase_status(int done) { return done == 3 ? NUMERICAL : (done == 0 ? ITER_LIMIT : OPEN); }
// phase 1 minimises a sum bounded below by 0: a ray there is an end like any other, the infeasibility left decides
inline int phase1_status(int done) { return phase_status(done); }
inline int phase2_status(int done) { return done == 2 ? UNBOUNDED : phase_status(done); }

} // namespace sx_spx_plan
