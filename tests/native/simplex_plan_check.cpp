// Stand-alone check of the dense simplex driver's host arithmetic (smart-crossover_amd/csrc/sx_simplex_plan.h).  Prints the
// violated expectation and exits with status 1; prints OK otherwise.  Built by tests/test_simplex_plan_cpu.py with the host
// sanitizers; includes nothing but the plan.  Arrays the plan reads live in exactly sized heap vectors, so that an index
// one past the end is a finding of the sanitizer and not a lucky read.
//
//   simplex_plan_check kept_head | round_trip | refresh | arena | fold | misc
#include "sx_simplex_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

namespace pl = sx_spx_plan;

[[noreturn]] static void fail(const char *what, long long a = 0, long long b = 0) {
    std::printf("VIOLATED: %s (%lld, %lld)\n", what, a, b);
    std::exit(1);
}
#define CHECK(cond, what, a, b)                                                                                                    \
    do {                                                                                                                           \
        if (!(cond)) fail(what, static_cast<long long>(a), static_cast<long long>(b));                                             \
    } while (0)

using Ids = std::vector<int64_t>;
using Codes = std::vector<int8_t>;
using Head = std::vector<int32_t>;
constexpr int8_t B = 0, L = -1, U = -2; // basic, at lower, at upper

static bool match(const Ids &head_ids, const Codes &vb, const Codes &cb, const Ids &col_ids, Head &head_new) {
    CHECK(vb.size() == col_ids.size(), "the case itself: one id per column", vb.size(), col_ids.size());
    return pl::match_kept_head(head_ids, vb.empty() ? nullptr : vb.data(), cb.empty() ? nullptr : cb.data(),
                               col_ids.empty() ? nullptr : col_ids.data(), static_cast<int64_t>(vb.size()),
                               static_cast<int64_t>(cb.size()), head_new);
}
static void expect_match(const char *what, const Ids &head_ids, const Codes &vb, const Codes &cb, const Ids &col_ids, const Head &want) {
    Head got;
    CHECK(match(head_ids, vb, cb, col_ids, got), what, 0, 0);
    CHECK(got.size() == want.size(), what, got.size(), want.size());
    for (size_t i = 0; i < want.size(); ++i) CHECK(got[i] == want[i], what, i, got[i]);
}
static void expect_refused(const char *what, const Ids &head_ids, const Codes &vb, const Codes &cb, const Ids &col_ids) {
    Head got;
    CHECK(!match(head_ids, vb, cb, col_ids, got), what, 0, 0);
}

// The inverse was left with head (id 12, logical of row 1, id 10, id 14) over four rows.  This round the columns come in
// another order and with one more: position -> id.
static void kept_head() {
    const Ids head = {12, -2, 10, 14};
    const Ids ids = {14, 99, 10, 12, 11, 13};
    expect_match("accepted under a permutation of the columns", head, {B, L, B, B, L, U}, {L, B, L, L}, ids, {3, 6 + 1, 2, 0});
    // id 10 no longer basic: once with a basic count of 3, once with row 0's logical making up the count
    expect_refused("a basic column missing (count short)", head, {B, L, L, B, L, U}, {L, B, L, L}, ids);
    expect_refused("a basic column missing (count made up by a logical)", head, {B, L, L, B, L, U}, {B, B, L, L}, ids);
    // id 99 basic on top: count 5; and with the count kept at 4 by dropping the logical of row 1
    expect_refused("a basic column extra (count over)", head, {B, B, B, B, L, U}, {L, B, L, L}, ids);
    expect_refused("a basic column extra (a logical of the head gone instead)", head, {B, B, B, B, L, U}, {L, L, L, L}, ids);
    // a head that names row 1 twice: count 4 and every position finds something, but basic column 12 serves none
    expect_refused("a basic column left over", {-2, -2, 10, 14}, {B, L, B, B, L, U}, {L, B, L, L}, ids);
    expect_refused("two basic columns with one id (count over)", head, {B, L, B, B, B, U}, {L, B, L, L}, {14, 99, 10, 12, 10, 13});
    expect_refused("two basic columns with one id (id 12 gone instead)", {12, -2, 10}, {L, L, B, B, L, L}, {L, B, L},
                   {14, 99, 10, 10, 11, 13});
    // count 3 = m and both positions of the head could find "a" column 10: only one of the two is remembered
    expect_refused("two basic columns with one id, named twice by the head", {10, -2, 10}, {L, L, B, B, L, L}, {L, B, L},
                   {14, 99, 10, 10, 11, 13});
    expect_refused("the head names an id twice", {12, 12, 10, 14}, {B, L, B, B, L, U}, {L, B, L, L}, ids);
    expect_refused("a logical whose row is now non-basic", head, {B, L, B, B, L, U}, {B, L, L, L}, ids);
    // -(4 + 1): row index m; the count is made up by row 0 so that only the range test can refuse
    expect_refused("a logical row index equal to m", {12, -5, 10, 14}, {B, L, B, B, L, U}, {B, L, L, L}, ids);
    expect_refused("a logical row index far past m", {12, -4000000000LL, 10, 14}, {B, L, B, B, L, U}, {B, L, L, L}, ids);
    expect_refused("head_ids one short", {12, -2, 10}, {B, L, B, B, L, U}, {L, B, L, L}, ids);
    expect_refused("head_ids one long", {12, -2, 10, 14, -1}, {B, L, B, B, L, U}, {L, B, L, L}, ids);
    expect_refused("head_ids empty", {}, {B, L, B, B, L, U}, {L, B, L, L}, ids);
    // heads of 3, 5 and 6 positions
    expect_match("three positions", {7, 8, 9}, {B, B, B}, {L, L, L}, {9, 8, 7}, {2, 1, 0});
    expect_match("five positions, all logical", {-5, -4, -3, -2, -1}, {L, U}, {B, B, B, B, B}, {1, 2}, {2 + 4, 2 + 3, 2 + 2, 2 + 1, 2 + 0});
    expect_match("six positions", {0, -1, 5, -6, 3, -3}, {L, B, L, B, B}, {B, L, B, L, L, B}, {4, 5, 2, 0, 3}, {3, 5 + 0, 1, 5 + 5, 4, 5 + 2});
    // m = 1
    expect_match("m = 1, the logical", {-1}, {L, U}, {B}, {5, 7}, {2});
    expect_match("m = 1, a column", {7}, {L, B}, {L}, {5, 7}, {1});
    expect_refused("m = 1, another column", {7}, {B, L}, {L}, {5, 7});
    expect_refused("m = 1, nothing basic", {-1}, {L, L}, {L}, {5, 7});
    // n = 0
    expect_match("n = 0", {-3, -1, -2}, {}, {B, B, B}, {}, {2, 0, 1});
    expect_refused("n = 0, the head names a column", {-3, 4, -2}, {}, {B, B, B}, {});
    expect_refused("n = 0, a row non-basic", {-3, -1, -2}, {}, {B, L, B}, {});
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd(uint64_t below) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (rng_state >> 33) % below;
}
template <class T>
static void shuffle(std::vector<T> &v) {
    for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[rnd(i)]);
}

// head -> ids -> (columns shuffled, some added) -> head: the same variables at the same positions
static void round_trip() {
    for (int64_t m = 3; m <= 6; ++m)
        for (int rep = 0; rep < 50; ++rep) {
            const int64_t n = m + 3;
            Ids col_ids(static_cast<size_t>(n));
            for (int64_t j = 0; j < n; ++j) col_ids[static_cast<size_t>(j)] = 1000 + 7 * j;
            Head vars(static_cast<size_t>(n + m));
            std::iota(vars.begin(), vars.end(), 0);
            shuffle(vars);
            const Head head(vars.begin(), vars.begin() + m); // m distinct variables in a random order
            Ids ids;
            pl::head_ids_of(head, col_ids.data(), n, ids);
            CHECK(static_cast<int64_t>(ids.size()) == m, "head_ids_of: one id per position", ids.size(), m);
            // next round: two more columns, all in a new order
            Ids next_ids = col_ids;
            next_ids.push_back(5);
            next_ids.push_back(6);
            shuffle(next_ids);
            const int64_t n2 = n + 2;
            Codes vb(static_cast<size_t>(n2), L), cb(static_cast<size_t>(m), L);
            for (int32_t k : head) {
                if (k >= n) cb[static_cast<size_t>(k - n)] = B;
                else
                    for (int64_t j = 0; j < n2; ++j)
                        if (next_ids[static_cast<size_t>(j)] == col_ids[static_cast<size_t>(k)]) vb[static_cast<size_t>(j)] = B;
            }
            Head head_new;
            CHECK(match(ids, vb, cb, next_ids, head_new), "round trip refused", m, rep);
            for (int64_t i = 0; i < m; ++i) {
                const int32_t k = head[static_cast<size_t>(i)], k2 = head_new[static_cast<size_t>(i)];
                if (k >= n) CHECK(k2 - n2 == k - n, "round trip: another row's logical", i, k2);
                else CHECK(k2 < n2 && next_ids[static_cast<size_t>(k2)] == col_ids[static_cast<size_t>(k)], "round trip: another column", i, k2);
            }
        }
    // without ids every structural is remembered as 0, a logical as ever
    Ids ids;
    pl::head_ids_of({2, 4, 0}, nullptr, 3, ids);
    CHECK(ids.size() == 3 && ids[0] == 0 && ids[1] == -2 && ids[2] == 0, "head_ids_of without col_ids", ids[1], ids[2]);
}

// 64 (m / 2048)^2 = m^2 / 65536, rounded down to a multiple of 64, clamped to 64 .. 2048 -- in integers:
//   m = 1, 2047: below 64 -> 64;  2048: 64;  2896: 8386816 / 65536 = 127.97 -> 64 (2897: 128.06 -> 128);
//   11585: 134212225 / 65536 = 2047.92 -> 1984 (11586: 2048.27 -> 2048);  10^6: clamped to 2048
static void refresh() {
    const long long want[][2] = {{1, 64}, {2047, 64}, {2048, 64}, {2896, 64}, {2897, 128}, {11585, 1984}, {11586, 2048}, {1000000, 2048}};
    for (const auto &w : want) CHECK(pl::refresh_interval(w[0]) == w[1], "refresh_interval", w[0], pl::refresh_interval(w[0]));
    CHECK(pl::refresh_interval(INT64_MAX) == 2048, "refresh_interval at the largest m", 0, 0);
}

// the requests of spx_allocate (and the head of spx_try_kept_inverse) in its order, each rounded up to 256 bytes
static size_t replay_requests(int64_t m, int64_t n, int64_t n_csc_tiles, bool has_session, bool defer, bool devex) {
    const size_t um = static_cast<size_t>(m), uN = static_cast<size_t>(n + m);
    size_t sum = 0;
    auto get = [&](size_t elem, size_t count) { sum += (elem * (count ? count : 1) + 255) & ~static_cast<size_t>(255); };
    auto grid1d = [](int64_t items, int64_t cap) {
        const int64_t g = (items + pl::WG - 1) / pl::WG;
        return static_cast<size_t>(g > cap ? cap : (g < 1 ? 1 : g));
    };
    get(1, uN), get(1, uN);                             // status, relaxed
    get(8, uN), get(8, uN), get(8, uN), get(8, uN);     // lo, up, cost, x
    if (devex) get(8, uN);                              // w
    get(4, um);                                         // head
    get(8, um), get(8, um), get(8, um), get(8, um);     // y, d, rho, rhs
    get(8, um);                                         // s_keep
    if (!has_session) get(8, um * um);                  // Binv
    if (defer) get(8, um * pl::DEFER), get(8, um * pl::DEFER), get(4, pl::DEFER); // E, R, er
    const size_t ratio_slots = grid1d(m, 4096);
    get(8, 3 * ratio_slots), get(4, 2 * ratio_slots), get(4, 2); // rt_val, rt_idx, tickets
    get(256, 1);                                        // st (the driver asserts sizeof(SpxState) <= 256)
    const size_t gP = static_cast<size_t>(n_csc_tiles < pl::GRID ? (n_csc_tiles > 0 ? n_csc_tiles : 1) : pl::GRID);
    const size_t gL = grid1d(m, 64);
    get(8, gP + gL), get(8, gP + gL), get(8, gP + gL);  // p_score, p_rc, p_idx
    get(8, 3);                                          // meas
    get(8, 2);                                          // resid_dev
    get(1, static_cast<size_t>(n)), get(1, um);         // vb_now, cb_now
    if (has_session) get(4, um);                        // head_dev of a kept inverse
    return sum;
}
static void arena() {
    for (int64_t m : {1, 63, 64, 1000})
        for (int64_t n : {int64_t(0), m, 5 * m / 2, 40 * m})
            for (int64_t tiles : {int64_t(0), n / pl::WG + 1, int64_t(100000)})
                for (int flags = 0; flags < 8; ++flags) {
                    const bool defer = flags & 1, devex = flags & 2, has_session = flags & 4;
                    const size_t have = pl::arena_bytes(m, n + m, has_session, defer, devex, pl::GRID);
                    const size_t need = replay_requests(m, n, tiles, has_session, defer, devex);
                    CHECK(have >= need, "arena_bytes below the sum of the requests", m * 1000000 + n, flags);
                    // ... and not a different order of magnitude: within the inverse-free part twice over
                    CHECK(have <= 2 * need + (1u << 16), "arena_bytes far above the requests", m * 1000000 + n, flags);
                }
}

static void fold() {
    // m: column tiles = ceil(m / 64); scalar grid = ceil(m / 256) * tiles; nkt = ceil(m / 16); nic = ceil(m / 256);
    // matrix-core grid = ceil(nkt / 64) * ceil(nic / 16) * 1024
    const long long want[][6] = {{1, 1, 1, 1, 1, 1024},     {15, 1, 1, 1, 1, 1024},   {16, 1, 1, 1, 1, 1024},   {255, 4, 4, 16, 1, 1024},
                                 {256, 4, 4, 16, 1, 1024},  {257, 5, 10, 17, 2, 1024}, {1025, 17, 85, 65, 5, 2048}, {4097, 65, 1105, 257, 17, 10240}};
    for (const auto &w : want) {
        const int64_t m = w[0];
        CHECK(pl::fold_col_tiles(m) == w[1], "fold_col_tiles", m, pl::fold_col_tiles(m));
        CHECK(pl::fold_grid(m) == w[2], "fold_grid", m, pl::fold_grid(m));
        CHECK(pl::fm_nkt(m) == w[3], "fm_nkt", m, pl::fm_nkt(m));
        CHECK(pl::fm_nic(m) == w[4], "fm_nic", m, pl::fm_nic(m));
        CHECK(pl::fm_grid(m) == w[5], "fm_grid", m, pl::fm_grid(m));
        // every entry of the inverse has a workgroup
        CHECK(static_cast<int64_t>(pl::fold_col_tiles(m)) * pl::FOLD_COLS >= m, "fold: columns uncovered", m, 0);
        CHECK(static_cast<int64_t>(pl::fold_grid(m) / pl::fold_col_tiles(m)) * pl::WG >= m, "fold: rows uncovered", m, 0);
        CHECK(static_cast<int64_t>(pl::fm_grid(m)) >= pl::fm_nkt(m) * pl::fm_nic(m), "matrix-core fold: tiles uncovered", m, 0);
    }
}

static void misc() {
    CHECK(pl::default_max_iter(0, 0) == 1000 && pl::default_max_iter(100, 250) == 18500, "default_max_iter", 0, 0);
    // m = 1000, N = 3500: 8e6 + 6e5 + 1.4e5 = 8.74e6 bytes; fits when 0.9 * free reaches that
    CHECK(pl::inverse_bytes(1000, 3500) == 8740000.0, "inverse_bytes", 0, 0);
    CHECK(pl::inverse_fits(1000, 3500, 9711112) && !pl::inverse_fits(1000, 3500, 9711110), "inverse_fits at the edge", 0, 0);
    CHECK(!pl::inverse_fits(200000, 700000, size_t(288) << 30), "3.2e11 bytes do not fit 288 GiB", 0, 0);
    // done: 0 running at the budget, 1 no candidate, 2 unbounded, 3 breakdown -> status 3, open, 2 (phase 2 only), 4
    const int p1[4] = {pl::ITER_LIMIT, pl::OPEN, pl::OPEN, pl::NUMERICAL}, p2[4] = {pl::ITER_LIMIT, pl::OPEN, pl::UNBOUNDED, pl::NUMERICAL};
    for (int done = 0; done < 4; ++done) {
        CHECK(pl::phase1_status(done) == p1[done], "phase1_status", done, pl::phase1_status(done));
        CHECK(pl::phase2_status(done) == p2[done], "phase2_status", done, pl::phase2_status(done));
    }
    CHECK(pl::OPEN == -1 && pl::OPTIMAL == 0 && pl::INFEASIBLE == 1 && pl::UNBOUNDED == 2 && pl::ITER_LIMIT == 3 && pl::NUMERICAL == 4,
          "the status codes of sx_simplex_result", 0, 0);
}

int main(int argc, char **argv) {
    const char *which = argc > 1 ? argv[1] : "";
    if (!std::strcmp(which, "kept_head")) kept_head();
    else if (!std::strcmp(which, "round_trip")) round_trip();
    else if (!std::strcmp(which, "refresh")) refresh();
    else if (!std::strcmp(which, "arena")) arena();
    else if (!std::strcmp(which, "fold")) fold();
    else if (!std::strcmp(which, "misc")) misc();
    else {
        std::printf("unknown case '%s'\n", which);
        return 2;
    }
    std::printf("OK\n");
    return 0;
}
