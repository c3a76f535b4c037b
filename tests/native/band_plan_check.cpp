// Stand-alone check of the sparse crossover's host set-up (smart-crossover_amd/csrc/sx_band_plan.h): reads a small LP from
// raw files, walks the plan's stages in the driver's order -- with a made-up outcome of the two LUs where the driver would
// ask the device -- and checks the invariants the stages promise each other.  Prints the violated invariant and exits
// with status 1.  Built by tests/test_band_plan_cpu.py with the host sanitizers; includes nothing but the plan.
//
//   band_plan_check DIR [blocks=K] [expect_P=K] [expect_cm=1] [basis=given] [lu=synthetic] [perturb=few|slack|many]
//                       [schur=synthetic] [write_basis=1] [expect=FILE]
#include "sx_band_plan.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>

namespace pl = sx_plan;

[[noreturn]] static void fail(const char *what, long long a = 0, long long b = 0) {
    std::printf("VIOLATED: %s (%lld, %lld)\n", what, a, b);
    std::exit(1);
}
#define CHECK(cond, what, a, b)                                                                                                    \
    do {                                                                                                                           \
        if (!(cond)) fail(what, static_cast<long long>(a), static_cast<long long>(b));                                             \
    } while (0)

template <class T>
static std::vector<T> slurp(const std::string &path, bool optional = false) {
    std::vector<T> v;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) {
        if (optional) return v;
        std::printf("cannot open %s\n", path.c_str());
        std::exit(2);
    }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize(static_cast<size_t>(bytes) / sizeof(T));
    if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(2);
    std::fclose(f);
    return v;
}
template <class T>
static void dump(const std::string &path, const std::vector<T> &v) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size())) std::exit(2);
    std::fclose(f);
}

// "name v v v ..." lines of the hand-written case
static std::map<std::string, std::vector<long long>> read_expect(const std::string &path) {
    std::map<std::string, std::vector<long long>> e;
    FILE *f = std::fopen(path.c_str(), "r");
    if (!f) std::exit(2);
    char line[4096];
    while (std::fgets(line, sizeof(line), f)) {
        char *tok = std::strtok(line, " \n");
        if (!tok) continue;
        std::vector<long long> &v = e[tok];
        while ((tok = std::strtok(nullptr, " \n"))) v.push_back(std::atoll(tok));
    }
    std::fclose(f);
    return e;
}
template <class T>
static void expect_eq(const std::map<std::string, std::vector<long long>> &e, const char *name, const std::vector<T> &got) {
    const auto it = e.find(name);
    if (it == e.end()) return;
    CHECK(it->second.size() == got.size(), name, it->second.size(), got.size());
    for (size_t k = 0; k < got.size(); ++k)
        if (it->second[k] != static_cast<long long>(got[k])) {
            std::printf("expected %s[%zu] = %lld, got %lld\n", name, k, it->second[k], static_cast<long long>(got[k]));
            fail(name, static_cast<long long>(k), static_cast<long long>(got[k]));
        }
}

// |a_ij| of column j in row i (0 when there is no entry)
static double entry(const pl::Csc &A, int64_t i, int64_t j) {
    for (int64_t k = A.ptr[j]; k < A.ptr[j + 1]; ++k)
        if (A.idx[k] == i) return std::fabs(A.val[k]);
    return 0.0;
}

// after the matching (positions before the cut)
static void check_matching(const pl::Csc &A, const pl::RowPlan &rp, const std::vector<uint8_t> &is_basic, const pl::Matching &mt) {
    const int64_t n = A.n, m1 = static_cast<int64_t>(rp.rows_band.size());
    std::vector<int64_t> pos_of(static_cast<size_t>(n + A.m), -1);
    for (int64_t p = 0; p < m1; ++p) {
        const int64_t v = mt.bvar[p];
        if (v < 0) continue;
        CHECK(v < n + A.m && is_basic[v], "a band position holds a variable that is not basic", p, v);
        CHECK(pos_of[v] < 0, "a variable holds two band positions", v, p);
        pos_of[v] = p;
        CHECK(mt.placed[v], "a variable on a band position is not marked placed", v, p);
        if (v < n) CHECK(entry(A, rp.rows_band[p], v) > pl::MATCH_MIN, "a column sits on a row where it has no entry above 1e-6", v, rp.rows_band[p]);
        else CHECK(v - n == rp.rows_band[p], "a logical sits on a row that is not its own", v - n, rp.rows_band[p]);
    }
    for (int64_t v = 0; v < n + A.m; ++v) CHECK(!mt.placed[v] || pos_of[v] >= 0, "a variable is marked placed without a position", v, 0);
    for (int64_t j = 0; j < n; ++j) {
        if (!is_basic[j] || mt.placed[j]) continue;
        for (int64_t k = A.ptr[j]; k < A.ptr[j + 1]; ++k) {
            const int32_t ib = rp.rowb[A.idx[k]];
            if (ib >= 0 && std::fabs(A.val[k]) > pl::MATCH_MIN)
                CHECK(mt.bvar[ib] >= 0, "an unplaced basic column still has an eligible entry in a free band row", j, A.idx[k]);
        }
    }
}

static int64_t block_of(const pl::EpochGeometry &g, int64_t p) { return std::min<int64_t>(p / g.stride, g.P - 1); }

static void check_geometry(const pl::Csc &A, const pl::RowPlan &rp, const pl::Matching &mt, const pl::EpochGeometry &g, const pl::BandTriplets &t) {
    const int64_t m = A.m, n = A.n;
    CHECK(g.m1 == (g.P - 1) * g.stride + g.RL_last && g.RL_last > 0, "band positions do not add up", g.m1, g.RL_last);
    CHECK(g.ndr == static_cast<int64_t>(rp.rows_dense.size()) + (g.P - 1) * g.Wsep, "border rows do not add up", g.ndr, g.Wsep);
    CHECK(static_cast<int64_t>(g.bvar.size()) == g.m1 && static_cast<int64_t>(g.rows_dense.size()) == g.ndr, "sizes of the geometry", g.m1, g.ndr);
    // eqidx: the m rows one-to-one onto the non-padding positions followed by the border rows
    std::vector<int32_t> row_at(static_cast<size_t>(g.m1 + g.ndr), -1);
    for (int64_t i = 0; i < m; ++i) {
        const int64_t q = g.eqidx[i];
        CHECK(q >= 0 && q < g.m1 + g.ndr, "eqidx out of range", i, q);
        CHECK(row_at[q] < 0, "eqidx maps two rows to one position", i, q);
        row_at[q] = static_cast<int32_t>(i);
        if (q < g.m1) CHECK(g.posrow[q] == i && g.rowb[i] == q, "eqidx, posrow and rowb disagree", i, q);
        else CHECK(g.rows_dense[q - g.m1] == i && g.rowb[i] == -1, "eqidx and rows_dense disagree", i, q);
    }
    int64_t npad = 0;
    for (int64_t p = 0; p < g.m1; ++p) {
        if (g.posrow[p] >= 0) {
            CHECK(row_at[p] == g.posrow[p], "a band position's row is not mapped to it", p, g.posrow[p]);
            CHECK(g.old_of_new[p] >= 0 && g.bvar[p] == mt.bvar[g.old_of_new[p]] && g.bvar[p] >= -1, "a position lost its variable in the cut", p, g.bvar[p]);
        } else {
            CHECK(g.bvar[p] == -2 && g.old_of_new[p] == -1, "a padding position does not carry -2", p, g.bvar[p]);
            ++npad;
        }
    }
    CHECK(npad == (g.P - 1) * g.PAD, "padding positions", npad, (g.P - 1) * g.PAD);
    for (int64_t k = 0; k < g.ndr; ++k) CHECK(row_at[g.m1 + k] >= 0, "a border row holds no row", k, 0);
    // the separators' columns left the band, the others kept their mark
    for (int64_t p = 0; p < g.m1_all; ++p)
        if (mt.bvar[p] >= 0) CHECK(mt.placed[mt.bvar[p]] == (g.rowb[rp.rows_band[p]] >= 0), "placed does not follow the cut", p, mt.bvar[p]);
    // triplets
    std::vector<int32_t> units(static_cast<size_t>(g.m1), 0), in_row(static_cast<size_t>(g.m1), 0);
    for (size_t e = 0; e < t.val.size(); ++e) {
        const int64_t r = t.row[e], c = t.col[e];
        CHECK(r >= 0 && r < g.m1 && c >= 0 && c < g.m1, "a triplet outside the band matrix", r, c);
        CHECK(r - c <= t.kl && c - r <= t.ku, "a triplet outside kl / ku", r, c);
        if (g.P > 1) CHECK(block_of(g, r) == block_of(g, c), "a triplet's row lies in another block than its column", r, c);
        CHECK(g.posrow[r] >= 0 || r == c, "a column reaches into a padding row", r, c);
        ++in_row[r];
        const int64_t v = g.bvar[c];
        if (v < 0 || v >= n) {
            CHECK(r == c && t.val[e] == 1.0, "a placeholder, logical or padding position is no unit column", c, v);
            ++units[c];
        }
    }
    for (int64_t p = 0; p < g.m1; ++p) {
        const int64_t v = g.bvar[p];
        if (v < 0 || v >= n) CHECK(units[p] == 1, "a unit column has not exactly one triplet", p, units[p]);
        if (g.posrow[p] < 0) CHECK(in_row[p] == 1, "a padding row holds more than its unit entry", p, in_row[p]);
    }
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string dir = std::string(argv[1]) + "/";
    std::map<std::string, std::string> opt;
    for (int a = 2; a < argc; ++a) {
        const std::string s = argv[a];
        const size_t eq = s.find('=');
        if (eq == std::string::npos) return 2;
        opt[s.substr(0, eq)] = s.substr(eq + 1);
    }
    auto has = [&](const char *k, const char *v) { return opt.count(k) && opt[k] == v; };
    const auto cptr = slurp<int64_t>(dir + "cptr.i64"), rptr = slurp<int64_t>(dir + "rptr.i64");
    const auto cidx = slurp<int32_t>(dir + "cidx.i32"), ridx = slurp<int32_t>(dir + "ridx.i32");
    const auto cval = slurp<double>(dir + "cval.f64"), lo = slurp<double>(dir + "lo.f64"), up = slurp<double>(dir + "up.f64");
    const auto rhs = slurp<double>(dir + "b.f64"), x = slurp<double>(dir + "x.f64"), slack = slurp<double>(dir + "slack.f64");
    const auto lt = slurp<uint8_t>(dir + "lt.u8");
    const int64_t n = static_cast<int64_t>(cptr.size()) - 1, m = static_cast<int64_t>(rptr.size()) - 1, nnz = static_cast<int64_t>(cval.size());
    CHECK(n > 0 && m > 0 && cptr[n] == nnz && rptr[m] == nnz && static_cast<int64_t>(lt.size()) == m && static_cast<int64_t>(x.size()) == n, "input files", m, n);
    const pl::Csc A{m, n, cptr.data(), cidx.data(), cval.data()};
    std::map<std::string, std::vector<long long>> expect;
    if (opt.count("expect")) expect = read_expect(opt["expect"]);

    // ---- rows
    pl::RowPlan rp;
    const int64_t thr = pl::dense_threshold(nnz, m);
    pl::classify_rows(m, rptr.data(), thr, rp);
    for (int32_t r : rp.rows_dense) CHECK(rptr[r + 1] - rptr[r] > thr, "a row below the threshold is called dense", r, thr);
    for (int32_t r : rp.rows_band) CHECK(rptr[r + 1] - rptr[r] <= thr, "a row above the threshold is in the band", r, thr);
    CHECK(static_cast<int64_t>(rp.rows_dense.size()) <= pl::MAX_NB, "dense rows", rp.rows_dense.size(), 0);
    const int64_t m1_all = static_cast<int64_t>(rp.rows_band.size());
    const int32_t tall_nat = pl::tallest(A, rp.rows_band);
    bool took_cm = false;
    if (tall_nat > pl::CM_TRIGGER && m1_all > 1) {
        std::vector<int32_t> cm;
        if (pl::cuthill_mckee_order(A, rptr.data(), ridx.data(), nnz, rp.rows_band, cm)) {
            std::vector<int32_t> a(rp.rows_band), b(cm);
            std::sort(a.begin(), a.end());
            std::sort(b.begin(), b.end());
            CHECK(a == b, "the Cuthill-McKee order is no permutation of the band rows", a.size(), b.size());
            const int32_t tall_cm = pl::tallest(A, cm);
            std::printf("tallest column: %d natural, %d Cuthill-McKee\n", tall_nat, tall_cm);
            if (tall_cm < tall_nat) {
                rp.rows_band = cm;
                took_cm = true;
            }
        }
    }
    if (has("expect_cm", "1")) {
        CHECK(tall_nat > pl::CM_TRIGGER, "the shuffled case does not reach the Cuthill-McKee trigger", tall_nat, pl::CM_TRIGGER);
        CHECK(took_cm && pl::tallest(A, rp.rows_band) <= tall_nat, "the plan did not take the Cuthill-McKee order", tall_nat, took_cm);
    }
    pl::finish_row_plan(m, rp);
    for (int64_t k = 0; k < m1_all; ++k) CHECK(rp.rowb[rp.rows_band[k]] == k && rp.eqidx[rp.rows_band[k]] == k, "row plan maps", k, 0);
    for (size_t k = 0; k < rp.rows_dense.size(); ++k)
        CHECK(rp.rowb[rp.rows_dense[k]] == -1 && rp.eqidx[rp.rows_dense[k]] == m1_all + static_cast<int64_t>(k), "a dense row is not in the border", k, 0);

    // ---- the first basic set
    pl::BasisState bs;
    bs.hx = x;
    for (int64_t j = 0; j < n; ++j) bs.hx[j] = std::min(std::max(bs.hx[j], lo[j]), up[j]);
    bs.init(n, m);
    const bool given = has("basis", "given");
    if (given) {
        const auto vb = slurp<int8_t>(dir + "vb.i8"), cb = slurp<int8_t>(dir + "cb.i8");
        CHECK(static_cast<int64_t>(vb.size()) == n && static_cast<int64_t>(cb.size()) == m, "basis files", vb.size(), cb.size());
        pl::basic_set_from_codes(n, m, vb.data(), cb.data(), lo.data(), up.data(), bs);
        for (int64_t j = 0; j < n; ++j) {
            CHECK((vb[j] == 0) == (bs.is_basic[j] != 0), "code 0 and the basic set disagree", j, vb[j]);
            if (vb[j] == -2 && !std::isinf(up[j])) CHECK(bs.hx[j] == up[j], "code -2 does not rest at the upper bound", j, 0);
            if (vb[j] == -1 && !std::isinf(lo[j])) CHECK(bs.hx[j] == lo[j], "code -1 does not rest at the lower bound", j, 0);
            CHECK(!std::isinf(bs.hx[j]), "a resting value is infinite", j, vb[j]);
        }
        CHECK(static_cast<int64_t>(bs.tracked.size()) == std::count(vb.begin(), vb.end(), int8_t(-3)), "code -3 and the tracked columns disagree", bs.tracked.size(), 0);
    } else {
        const size_t ncand = pl::basic_set_from_margins(n, m, lo.data(), up.data(), rhs.data(), lt.data(), slack.data(), bs);
        const int64_t nbasic = std::count(bs.is_basic.begin(), bs.is_basic.end(), uint8_t(1));
        CHECK(nbasic == std::min<int64_t>(m, static_cast<int64_t>(ncand)) && nbasic + bs.tracked.size() == ncand, "candidates", nbasic, ncand);
        double least_in = INFINITY, most_out = -INFINITY;
        for (int64_t v = 0; v < n + m; ++v)
            if (bs.is_basic[v]) least_in = std::min(least_in, bs.margin[v]);
        for (int32_t v : bs.tracked) most_out = std::max(most_out, bs.margin[v]);
        CHECK(!(most_out > least_in), "a tracked candidate has a larger margin than a basic one", 0, 0);
    }
    if (opt.count("perturb")) { // a basic set with too few / too many members, as a given basis may be
        int64_t k = 0;
        if (has("perturb", "few")) // (the dense rows' own logicals leave too: the border is left short of columns)
            for (int32_t r : rp.rows_dense) bs.is_basic[n + r] = 0;
        if (has("perturb", "slack")) { // the band rows' logicals and nothing else: only the dense rows' logicals can fill the border
            std::fill(bs.is_basic.begin(), bs.is_basic.end(), 0);
            for (int32_t r : rp.rows_band) bs.is_basic[n + r] = 1;
            bs.tracked.erase(std::remove_if(bs.tracked.begin(), bs.tracked.end(), [&](int32_t v) { return bs.is_basic[v] != 0; }), bs.tracked.end());
        }
        for (int64_t j = 0; j < n; ++j) {
            if (has("perturb", "few") && bs.is_basic[j]) { // every tenth column, and every column that belongs to a dense row
                int64_t big = A.ptr[j];
                for (int64_t e = A.ptr[j]; e < A.ptr[j + 1]; ++e)
                    if (std::fabs(A.val[e]) > std::fabs(A.val[big])) big = e;
                if (++k % 10 == 0 || rp.rowb[A.idx[big]] < 0) bs.is_basic[j] = 0;
            }
            if (has("perturb", "many") && !bs.is_basic[j] && ++k % 50 == 0) {
                bs.is_basic[j] = 1;
                bs.tracked.erase(std::remove(bs.tracked.begin(), bs.tracked.end(), static_cast<int32_t>(j)), bs.tracked.end());
            }
        }
    }

    // ---- columns to rows, geometry, triplets
    pl::Matching mt;
    pl::match_columns_to_rows(A, rp, bs.is_basic, bs.prev_pos, mt);
    check_matching(A, rp, bs.is_basic, mt);
    expect_eq(expect, "matching", mt.bvar);
    const pl::Matching mt0 = mt;
    pl::EpochGeometry g;
    const int64_t want = opt.count("blocks") ? std::atoll(opt["blocks"].c_str()) : pl::default_block_count(m1_all);
    pl::make_geometry(A, rp, mt, want, g);
    pl::BandTriplets tri;
    pl::band_triplets(A, nnz, g, tri);
    std::printf("m=%lld n=%lld: %lld band rows, %lld dense; P=%lld RL=%lld Wsep=%lld PAD=%lld stride=%lld RL_last=%lld m1=%lld kl=%d ku=%d\n", (long long)m,
                (long long)n, (long long)m1_all, (long long)rp.rows_dense.size(), (long long)g.P, (long long)g.RL, (long long)g.Wsep, (long long)g.PAD,
                (long long)g.stride, (long long)g.RL_last, (long long)g.m1, tri.kl, tri.ku);
    {
        pl::Matching chk = mt0;
        chk.placed = mt.placed;
        check_geometry(A, rp, chk, g, tri);
    }
    if (opt.count("expect_P")) CHECK(g.P == std::atoll(opt["expect_P"].c_str()), "number of blocks", g.P, want);
    expect_eq(expect, "geometry", std::vector<int64_t>{g.P, g.RL, g.Wsep, g.PAD, g.stride, g.RL_last, g.m1, g.ndr, tri.kl, tri.ku});
    expect_eq(expect, "eqidx", g.eqidx);

    // ---- the band LU's outcome
    std::vector<int32_t> rep(static_cast<size_t>(g.m1), 0), piv(static_cast<size_t>(g.m1));
    std::iota(piv.begin(), piv.end(), 0);
    int64_t nrep = 0, nswap = 0;
    if (has("lu", "synthetic"))
        for (int64_t j = 0; j + 1 < g.m1; ++j) {
            if (j % 97 == 5 && g.bvar[j] >= 0 && g.bvar[j] < n) rep[j] = 1, ++nrep;
            else if (j % 53 == 7 && g.posrow[j] >= 0 && g.posrow[j + 1] >= 0 && tri.kl >= 1) piv[j] = static_cast<int32_t>(j + 1), ++nswap;
        }
    std::vector<int32_t> ph_row(static_cast<size_t>(g.m1), -1);
    const std::vector<int64_t> bvar_before = g.bvar;
    pl::after_band_lu(g, mt, rep, piv, ph_row);
    std::vector<uint8_t> row_used(static_cast<size_t>(m), 0);
    for (int64_t p = 0; p < g.m1; ++p) {
        if (g.bvar[p] == -1) {
            CHECK(ph_row[p] >= 0 && ph_row[p] < m && g.rowb[ph_row[p]] >= 0, "a placeholder without a band row", p, ph_row[p]);
            CHECK(!row_used[ph_row[p]], "two placeholders stand for one row", p, ph_row[p]);
            row_used[ph_row[p]] = 1;
            if (rep[p] && bvar_before[p] >= 0) CHECK(!mt.placed[bvar_before[p]], "a replaced column is still marked placed", p, bvar_before[p]);
        } else CHECK(ph_row[p] == -1 && g.bvar[p] == bvar_before[p], "the band LU's bookkeeping touched a position it kept", p, g.bvar[p]);
    }
    std::printf("band LU: %lld columns replaced, %lld row swaps\n", (long long)nrep, (long long)nswap);

    // ---- the border
    pl::Border bd;
    const std::vector<uint8_t> basic_before = bs.is_basic;
    const bool balanced = pl::balance_border(n, g, mt, ph_row, !given, bs, bd);
    int64_t filled_ph = 0, filled_dense = 0, surplus = 0; // which branches of the balancing ran
    for (int64_t v = 0; v < n + m; ++v) {
        if (bs.is_basic[v] && !basic_before[v]) {
            CHECK(v >= n, "the balancing made a column basic", v, 0);
            ++(g.rowb[v - n] >= 0 ? filled_ph : filled_dense);
        }
        if (!bs.is_basic[v] && basic_before[v]) {
            CHECK(std::count(bs.tracked.begin(), bs.tracked.end(), static_cast<int32_t>(v)) == 1, "a surplus column is not tracked", v, 0);
            ++surplus;
        }
    }
    std::printf("balancing: %lld placeholders became logicals, %lld logicals of border rows filled in, %lld columns went superbasic\n",
                (long long)filled_ph, (long long)filled_dense, (long long)surplus);
    CHECK(balanced, "the border does not balance", g.ndr + bd.h, bd.bcol.size());
    int64_t h = 0;
    for (int64_t p = 0; p < g.m1; ++p) h += g.bvar[p] == -1;
    CHECK(h == bd.h && static_cast<int64_t>(bd.ph_pos.size()) == h, "placeholders counted wrongly", h, bd.h);
    CHECK(static_cast<int64_t>(bd.bcol.size()) == g.ndr + h, "the border has not exactly ndr + h columns", bd.bcol.size(), g.ndr + h);
    for (int64_t v : bd.bcol) CHECK(v >= 0 && bs.is_basic[v] && !mt.placed[v], "a border column is not an unplaced basic variable", v, 0);
    for (int32_t v : bs.tracked) CHECK(!bs.is_basic[v], "a tracked column is basic after the border was balanced", v, 0);
    std::printf("border: %lld rows (%lld dense or separator, %lld placeholders)\n", (long long)(g.ndr + h), (long long)g.ndr, (long long)h);
    const int64_t nb = bd.nb(g);

    // ---- the dense LU's outcome
    std::vector<int32_t> rep2(static_cast<size_t>(nb), 0), perm2(static_cast<size_t>(nb));
    std::iota(perm2.begin(), perm2.end(), 0);
    if (has("schur", "synthetic")) { // one column whose diagonal is a dense row, one whose diagonal is a placeholder's row
        int64_t j_dense = -1, j_ph = -1;
        for (int64_t j = 0; j < g.ndr && j_dense < 0; ++j)
            if (!bs.is_basic[n + g.rows_dense[j]]) j_dense = j;
        for (int64_t j = g.ndr; j < nb && j_ph < 0; ++j)
            if (!bs.is_basic[n + ph_row[bd.ph_pos[j - g.ndr]]]) j_ph = j;
        CHECK(j_dense >= 0 && j_ph >= 0, "the case does not reach both repair branches of the dense LU", j_dense, j_ph);
        rep2[j_dense] = rep2[j_ph] = 1;
        const std::vector<int64_t> before = bd.bcol;
        const int64_t twice = pl::after_dense_lu(n, g, ph_row, rep2, perm2, bs, bd);
        CHECK(twice < 0, "the repair wants a logical twice", twice, 0);
        CHECK(bd.bcol[j_dense] == n + g.rows_dense[j_dense] && bd.bcol[j_ph] == -1, "the repair's border columns", bd.bcol[j_dense], bd.bcol[j_ph]);
        CHECK(g.bvar[bd.ph_pos[j_ph - g.ndr]] == n + ph_row[bd.ph_pos[j_ph - g.ndr]], "the placeholder did not become its row's logical", j_ph, 0);
        CHECK(!bs.is_basic[before[j_dense]] && !bs.is_basic[before[j_ph]], "a column without a pivot is still basic", before[j_dense], before[j_ph]);
        CHECK(std::count(bs.tracked.begin(), bs.tracked.end(), static_cast<int32_t>(before[j_dense])) == 1, "a column without a pivot is not tracked", before[j_dense], 0);
    } else CHECK(pl::after_dense_lu(n, g, ph_row, rep2, perm2, bs, bd) < 0, "after_dense_lu without a replaced column", 0, 0);

    // ---- B21, B12
    pl::HostRows b21r, b21c, b12r, b12c;
    if (nb > 0) {
        pl::b21_blocks(A, g, bd, b21r, b21c);
        CHECK(static_cast<int64_t>(b21r.ptr.size()) == nb + 1 && b21c.ptr.size() == b21c.list.size() + 1, "B21's shape", b21r.ptr.size(), b21c.ptr.size());
        for (int32_t p : b21r.idx) CHECK(p >= 0 && p < g.m1 && g.bvar[p] != -2, "B21 reaches outside the band or into padding", p, 0);
        for (int32_t r : b21c.idx) CHECK(r >= 0 && r < nb, "B21 reaches outside the border", r, 0);
        if (g.m1 > 0) {
            pl::b12_blocks(A, g, bd, b12r, b12c);
            CHECK(static_cast<int64_t>(b12c.ptr.size()) == nb + 1 && b12r.ptr.size() == b12r.list.size() + 1, "B12's shape", b12c.ptr.size(), b12r.ptr.size());
            for (int32_t p : b12c.idx) CHECK(p >= 0 && p < g.m1 && g.posrow[p] >= 0, "B12 reaches outside the band or into padding", p, 0);
            for (int32_t j : b12r.idx) CHECK(j >= 0 && j < nb && bd.bcol[j] >= 0, "B12 holds a column that is not in the border", j, 0);
        }
    }

    // ---- who is where
    std::vector<int64_t> head;
    std::vector<int32_t> varJ;
    int64_t n_dummy = 0, bad = 0;
    const int who = pl::who_is_where(m, g, bd, bs, head, varJ, n_dummy, bad);
    CHECK(who == 0, "who is where: a variable twice (1) or not m basic variables (2)", who, bad);
    std::vector<uint8_t> seen(static_cast<size_t>(n + m), 0);
    int64_t nbasic = 0;
    for (int64_t v : head) {
        if (v < 0) continue;
        CHECK(!seen[v], "a variable is basic twice", v, 0);
        seen[v] = 1;
        ++nbasic;
    }
    CHECK(nbasic == m && nbasic + n_dummy == static_cast<int64_t>(head.size()), "not exactly m basic variables", nbasic, m);
    for (int64_t v = 0; v < n + m; ++v) CHECK((bs.vstat[v] == 1) == (seen[v] != 0) && (bs.is_basic[v] != 0) == (seen[v] != 0), "vstat / is_basic do not follow head", v, bs.vstat[v]);
    for (size_t k = 0; k < varJ.size(); ++k) {
        CHECK(!seen[varJ[k]] && bs.vstat[varJ[k]] == 2, "a tracked column is basic", varJ[k], 0);
        if (k) CHECK(varJ[k - 1] < varJ[k], "tracked columns are not in ascending order", varJ[k - 1], varJ[k]);
    }
    expect_eq(expect, "head", head);
    expect_eq(expect, "varJ", varJ);
    std::printf("basis: %lld positions, %lld dummies, %zu tracked columns\n", (long long)head.size(), (long long)n_dummy, varJ.size());

    if (has("write_basis", "1")) { // the basic set as codes, for the given-basis case
        std::vector<int8_t> vb(static_cast<size_t>(n), -1), cb(static_cast<size_t>(m), -1);
        for (int64_t j = 0; j < n; ++j) vb[j] = seen[j] ? 0 : -1;
        for (int64_t i = 0; i < m; ++i) cb[i] = seen[n + i] ? 0 : -1;
        dump(dir + "vb.i8", vb);
        dump(dir + "cb.i8", cb);
    }
    std::printf("OK\n");
    return 0;
}
