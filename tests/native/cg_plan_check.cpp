// Stand-alone check of the projector CG's host arithmetic (smart-crossover_amd/csrc/sx_cg_plan.h).  Prints the violated
// expectation and exits with status 1; prints OK otherwise.  Built by tests/test_cg_plan_cpu.py with the host sanitizers;
// includes nothing but the plan.  Expected values are written out here, not taken from the plan's own constants.
//
//   cg_plan_check walk_grid | vector_grid | layout | stopping
#include "sx_cg_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

namespace pl = sx_cg_plan;

[[noreturn]] static void fail(const char *what, long long a = 0, long long b = 0) {
    std::printf("VIOLATED: %s (%lld, %lld)\n", what, a, b);
    std::exit(1);
}
#define CHECK(cond, what, a, b)                                                                                                    \
    do {                                                                                                                           \
        if (!(cond)) fail(what, static_cast<long long>(a), static_cast<long long>(b));                                             \
    } while (0)

// at most 2048, a multiple of 8 under the XCD map from 64 tiles on, never below 1
static void walk_grid() {
    const long long tiles[] = {0, 1, 63, 64, 65, 2047, 2048, 2049, 5000};
    const int want_on[] = {1, 1, 63, 64, 64, 2040, 2048, 2048, 2048};
    const int want_off[] = {1, 1, 63, 64, 65, 2047, 2048, 2048, 2048};
    for (int k = 0; k < 9; ++k) {
        CHECK(pl::walk_grid(tiles[k], true) == want_on[k], "walk grid, XCD map on", tiles[k], pl::walk_grid(tiles[k], true));
        CHECK(pl::walk_grid(tiles[k], false) == want_off[k], "walk grid, XCD map off", tiles[k], pl::walk_grid(tiles[k], false));
    }
}

// ceil(len / 1024) in 1 .. 1024 (4 elements per lane of 256)
static void vector_grid() {
    CHECK(pl::WG == 256, "lanes per workgroup", pl::WG, 256);
    const long long quad = 4 * 256;
    const long long len[] = {0, 1, quad, quad + 1, 1024 * quad, 1024 * quad + 1};
    const int want[] = {1, 1, 1, 2, 1024, 1024};
    for (int k = 0; k < 6; ++k) CHECK(pl::vector_grid(len[k]) == want[k], "vector grid", len[k], pl::vector_grid(len[k]));
}

static void layout() {
    const long long shapes[][2] = {{1, 0}, {1, 1}, {7, 3}, {1000, 5000}};
    for (const auto &mn : shapes) {
        const long long m = mn[0], n = mn[1], nn = n > 0 ? n : 1;
        const size_t vm = 8 * static_cast<size_t>(m), vn = 8 * static_cast<size_t>(nn);
        const pl::Layout L = pl::layout(m, n);
        // region = (offset, bytes): the state (48 bytes used of the 256 set aside), two partial arrays, z r p q, w atz
        const std::vector<std::pair<size_t, size_t>> regions = {
            {L.state, 48}, {L.ppq, 8 * 2048}, {L.prr, 8 * 2048}, {L.z, vm}, {L.r, vm}, {L.p, vm}, {L.q, vm}, {L.w, vn}, {L.atz, vn},
        };
        for (size_t i = 0; i < regions.size(); ++i) {
            CHECK(regions[i].first % 8 == 0, "a region is 8-byte aligned", m, i);
            CHECK(regions[i].first + regions[i].second <= L.bytes, "a region ends inside bytes", m, i);
            for (size_t j = 0; j < i; ++j) {
                const bool apart = regions[j].first + regions[j].second <= regions[i].first ||
                                   regions[i].first + regions[i].second <= regions[j].first;
                CHECK(apart, "two regions overlap", i, j);
            }
        }
        CHECK(L.atz > L.w && L.w > L.q, "atz is the last region", m, n);
        // what the drivers reserved before the plan existed: single device with n (>= 1 there), sharded with max(n, 1)
        const size_t off_vec = 256 + 2 * 8 * 2048;
        const size_t sharded = off_vec + 8 * (4 * static_cast<size_t>(m) + 2 * static_cast<size_t>(nn)) + 256;
        CHECK(L.bytes == sharded, "bytes equals the sharded driver's formula", L.bytes, sharded);
        if (n >= 1) {
            const size_t single = off_vec + 8 * (4 * static_cast<size_t>(m) + 2 * static_cast<size_t>(n)) + 256;
            CHECK(L.bytes == single, "bytes equals the single-device driver's formula", L.bytes, single);
        }
        CHECK(L.z == off_vec && L.w == off_vec + 8 * 4 * static_cast<size_t>(m), "z r p q, then w", L.z, L.w);
    }
}

static void expect_start(const char *what, const pl::Start &s, bool trivial, bool run, int done) {
    CHECK(s.trivial == trivial, what, s.trivial, trivial);
    CHECK(s.run == run, what, s.run, run);
    CHECK(s.done == done, what, s.done, done);
}

static void stopping() {
    const double tol = 1e-8;
    // ||b|| = 0 and ||b|| = tol: the legacy immediate exit, for both
    expect_start("single, b = 0", pl::start_single(0.0, tol), true, false, 1);
    expect_start("sharded, b = 0", pl::start_sharded(0.0, tol), true, false, 1);
    expect_start("single, b = tol", pl::start_single(tol, tol), true, false, 1);
    expect_start("sharded, b = tol", pl::start_sharded(tol, tol), true, false, 1);
    // just above: the loop runs, for both
    const double above = std::nextafter(tol, 1.0);
    expect_start("single, b just above tol", pl::start_single(above, tol), false, true, 0);
    expect_start("sharded, b just above tol", pl::start_sharded(above, tol), false, true, 0);
    // tol = 2 with ||b|| = 3 > tol: ||r|| < tol ||b|| holds before the first iteration, the one case in which the rules differ:
    // the single device skips the loop and leaves done = 0 (not trivial), the sharded rule reports trivial and sets done
    expect_start("single, tol = 2", pl::start_single(3.0, 2.0), false, false, 0);
    expect_start("sharded, tol = 2", pl::start_sharded(3.0, 2.0), true, false, 1);
    // and below tol = 2 both are trivial
    expect_start("single, tol = 2, b = 1", pl::start_single(1.0, 2.0), true, false, 1);
    expect_start("sharded, tol = 2, b = 1", pl::start_sharded(1.0, 2.0), true, false, 1);
    // a NaN norm never enters the loop
    expect_start("single, b = NaN", pl::start_single(std::nan(""), tol), true, false, 1);
    expect_start("sharded, b = NaN", pl::start_sharded(std::nan(""), tol), true, false, 1);

    // result values: rho[iters & 1] is the last r.r; b = 0 reports 0; trivial counts as converged
    const double rho[2] = {16.0, 4.0};
    CHECK(pl::rel_residual(rho, 0, 4.0) == 1.0, "rel_residual before the first iteration", 0, 0);
    CHECK(pl::rel_residual(rho, 7, 4.0) == 0.5, "rel_residual after an odd iteration", 7, 0);
    CHECK(pl::rel_residual(rho, 8, 4.0) == 1.0, "rel_residual after an even iteration", 8, 0);
    CHECK(pl::rel_residual(rho, 3, 0.0) == 0.0, "rel_residual with b = 0", 3, 0);
    CHECK(pl::converged(true, 0) == 1 && pl::converged(false, 0) == 0 && pl::converged(false, 1) == 1, "converged under trivial", 0, 0);
}

int main(int argc, char **argv) {
    const char *which = argc > 1 ? argv[1] : "";
    if (!std::strcmp(which, "walk_grid")) walk_grid();
    else if (!std::strcmp(which, "vector_grid")) vector_grid();
    else if (!std::strcmp(which, "layout")) layout();
    else if (!std::strcmp(which, "stopping")) stopping();
    else fail("usage: cg_plan_check walk_grid | vector_grid | layout | stopping");
    std::printf("OK\n");
    return 0;
}
