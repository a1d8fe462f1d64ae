// tests/hostcheck/cosetmixedcheck.cpp — TEST-ONLY driver for a plain g++ build of csrc/host_coset_mixed.h and the mixed scalars of
// csrc/host_coset_verify.h (no GPU, no library).  Over a grid of class tables and item counts, empty and repeated classes included, it checks
//   * the planner: every non-empty class of l <= 1024 gets between 1 and its tile count of workgroups, the total is at most 1 024, the
//     workgroup tables name their classes in contiguous runs, the rows tile the row-sum input exactly (plane rows then wire rows, no gap, no
//     overlap), the LDS of a launch is the largest of its classes and at most 55 KiB, the length groups partition the permutation;
//   * the permutation is a bijection sorted by (chunk length, class) and stable within a class, the offsets are prefix sums;
//   * the mixed scalars r_p | r_p w_s^(k l_s) | row sums against host_fr.h arithmetic done the slow way (square and multiply from w_s);
//   * the error order of mixed_checks, one case per step in front of a later fault.
// Prints "ok <checks>" and exits 0, or names the first failure and exits 1.  tests/test_multiproof_verify_mixed_host.py builds it plain and
// with ASan + UBSan as a stand-alone executable.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>

#include "host_coset_mixed.h"
#include "host_coset_verify.h"

using namespace kzg_host;

static size_t checks = 0;
#define CHECK(cond, ...)                                                                     \
    do {                                                                                     \
        ++checks;                                                                            \
        if (!(cond)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } \
    } while (0)

static void threads_for(size_t n, const std::function<void(size_t)>& job) {
    std::vector<std::thread> ts;
    for (size_t i = 1; i < n; ++i) ts.emplace_back([&job, i] { job(i); });
    if (n) job(0);
    for (auto& t : ts) t.join();
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

struct Case { std::vector<uint64_t> n, l, counts; };

static void check_plan(const Case& c, int tag) {
    const size_t S = c.n.size();
    std::vector<uint64_t> cls;
    for (size_t s = 0; s < S; ++s) for (uint64_t j = 0; j < c.counts[s]; ++j) cls.push_back(s);
    for (size_t i = cls.size(); i > 1; --i) std::swap(cls[i - 1], cls[rnd() % i]);           // the caller's order is arbitrary
    const size_t N = cls.size();
    MixedPlan p;
    mixed_plan(c.n.data(), c.l.data(), S, cls.data(), N, &p);
    // offsets: prefix sums in the caller's order
    size_t total = 0, l_max = 0;
    CHECK(p.val_off.size() == N && p.perm.size() == N, "case %d", tag);
    for (size_t i = 0; i < N; ++i) { CHECK(p.val_off[i] == total, "case %d item %zu", tag, i); total += c.l[cls[i]]; }
    CHECK(p.total_values == total, "case %d", tag);
    for (size_t s = 0; s < S; ++s) l_max = std::max<size_t>(l_max, c.l[s]);
    CHECK(p.l_max == l_max, "case %d", tag);
    // permutation: a bijection, sorted by (l, class), stable within a class; the class ranges cover it
    std::vector<int> seen(N, 0);
    for (size_t j = 0; j < N; ++j) { CHECK(p.perm[j] < N && !seen[p.perm[j]], "case %d slot %zu", tag, j); seen[p.perm[j]] = 1; }
    for (size_t j = 1; j < N; ++j) {
        const uint64_t a = cls[p.perm[j - 1]], b = cls[p.perm[j]];
        CHECK(c.l[a] < c.l[b] || (c.l[a] == c.l[b] && (a < b || (a == b && p.perm[j - 1] < p.perm[j]))), "case %d slot %zu", tag, j);
    }
    size_t covered = 0;
    int log_n_max = 0;
    for (size_t s = 0; s < S; ++s) {
        const MixedClassDev& d = p.cls[s];
        CHECK(d.count == c.counts[s], "case %d class %zu", tag, s);
        for (uint32_t j = 0; j < d.count; ++j) CHECK(cls[p.perm[d.first + j]] == s, "case %d class %zu", tag, s);
        covered += d.count;
        if (d.count) {
            CHECK(((uint64_t)1 << d.log_l) == c.l[s] && ((uint64_t)1 << d.log_n) == c.n[s], "case %d class %zu", tag, s);
            log_n_max = std::max(log_n_max, (int)d.log_n);
        }
    }
    CHECK(covered == N && p.log_n_max == log_n_max, "case %d", tag);
    // length groups: ascending, disjoint, cover the permutation, the G2 class is the first class of that length
    size_t at = 0;
    for (size_t g = 0; g < p.lens.size(); ++g) {
        const MixedLenGroup& lg = p.lens[g];
        CHECK(lg.first == at && lg.count > 0 && (g == 0 || p.lens[g - 1].l < lg.l), "case %d group %zu", tag, g);
        for (size_t j = 0; j < lg.count; ++j) CHECK(c.l[cls[p.perm[lg.first + j]]] == lg.l, "case %d group %zu", tag, g);
        size_t q = 0;
        while (c.l[q] != lg.l) ++q;
        CHECK(lg.g2_class == q, "case %d group %zu", tag, g);
        at += lg.count;
    }
    CHECK(at == N, "case %d", tag);
    // workgroups
    size_t wgs = 0, plane_rows = 0, words = 0;
    size_t lds[2] = {0, 0};
    for (size_t s = 0; s < S; ++s) {
        const MixedClassDev& d = p.cls[s];
        if (!d.count || c.l[s] > MIXED_LDS_MAX_L) { CHECK(d.tiles == 0 && d.wg_count == 0, "case %d class %zu", tag, s); continue; }
        const int launch = c.l[s] == 1024 ? 1 : 0;
        const uint32_t E = launch ? 1024 : 512, cpt = E / (uint32_t)c.l[s];
        CHECK(d.tiles == (d.count + cpt - 1) / cpt, "case %d class %zu", tag, s);
        CHECK(d.wg_count >= 1 && d.wg_count <= d.tiles, "case %d class %zu: %u workgroups for %u tiles", tag, s, d.wg_count, d.tiles);
        CHECK((size_t)d.wg_first + d.wg_count <= p.wg_class[launch].size(), "case %d class %zu", tag, s);
        for (uint32_t g = 0; g < d.wg_count; ++g) CHECK(p.wg_class[launch][d.wg_first + g] == s, "case %d class %zu", tag, s);
        wgs += d.wg_count;
        lds[launch] = std::max(lds[launch], mixed_interp_lds_bytes(E, c.l[s]));
    }
    CHECK(wgs == p.wg_class[0].size() + p.wg_class[1].size() && wgs <= MIXED_MAX_GROUPS, "case %d: %zu workgroups", tag, wgs);
    CHECK(lds[0] == p.lds_bytes[0] && lds[1] == p.lds_bytes[1] && lds[0] <= 55 * 1024 && lds[1] <= 55 * 1024, "case %d", tag);
    // rows: plane rows in the order of the classes' row_off, each class's rows one after the other; then the wire rows; exact tiling
    for (const MixedRow& r : p.rows) {
        if (r.log_l_kind & 0x100u) break;
        CHECK(r.off == words, "case %d plane row %zu", tag, plane_rows);
        words += 9 * ((size_t)1 << (r.log_l_kind & 0xFF));
        ++plane_rows;
    }
    CHECK(plane_rows == wgs && words == p.plane_words, "case %d", tag);
    for (size_t s = 0; s < S; ++s) {
        const MixedClassDev& d = p.cls[s];
        for (uint32_t g = 0; g < d.wg_count; ++g) {
            bool found = false;
            for (size_t r = 0; r < plane_rows; ++r)
                if (p.rows[r].off == d.row_off + g * 9 * c.l[s]) { found = (p.rows[r].log_l_kind == d.log_l); break; }
            CHECK(found, "case %d class %zu workgroup %u has no row", tag, s, g);
        }
    }
    size_t elems = 0, n_long = 0;
    for (size_t r = plane_rows; r < p.rows.size(); ++r) {
        CHECK((p.rows[r].log_l_kind & 0x100u) && p.rows[r].off == elems, "case %d wire row %zu", tag, r);
        const MixedLongItem& it = p.long_items[r - plane_rows];
        CHECK(it.row_off == elems && it.log_l == (p.rows[r].log_l_kind & 0xFF) && it.val_off == p.val_off[it.item], "case %d wire row %zu", tag, r);
        CHECK(c.l[cls[it.item]] == ((uint64_t)1 << it.log_l) && c.n[cls[it.item]] == ((uint64_t)1 << it.log_n), "case %d wire row %zu", tag, r);
        elems += (size_t)1 << it.log_l;
        ++n_long;
    }
    size_t want_long = 0;
    for (size_t s = 0; s < S; ++s) if (c.l[s] > MIXED_LDS_MAX_L) want_long += c.counts[s];
    CHECK(n_long == want_long && p.long_items.size() == n_long && elems == p.wire_elems, "case %d", tag);
}

// a^e by square and multiply (wire form)
static void fr_pow(const uint64_t a[4], uint64_t e, uint64_t out[4]) {
    uint64_t acc[4], base[4];
    fr_one(acc);
    for (int i = 0; i < 4; ++i) base[i] = a[i];
    for (; e; e >>= 1) { if (e & 1) fr_mul(acc, base, acc); fr_mul(base, base, base); }
    for (int i = 0; i < 4; ++i) out[i] = acc[i];
}

static void check_scalars(const Case& c, size_t M, int tag) {
    const size_t S = c.n.size();
    std::vector<uint64_t> cls, ks, rows;
    for (size_t s = 0; s < S; ++s) for (uint64_t j = 0; j < c.counts[s]; ++j) cls.push_back(s);
    for (size_t i = cls.size(); i > 1; --i) std::swap(cls[i - 1], cls[rnd() % i]);
    const size_t N = cls.size();
    std::vector<uint64_t> r(4 * N), class_m(S), out(4 * (2 * N + M), 0xdeadbeefULL);          // exactly the sizes the header is told
    for (size_t s = 0; s < S; ++s) class_m[s] = c.n[s] / c.l[s];
    for (size_t i = 0; i < N; ++i) {
        const uint64_t a = (uint64_t)(i + 1) * 0x9e3779b97f4a7c15ULL, x[4] = {a, ~a, 3 * a, (uint64_t)(i & 0xffff)};
        fr_mul(FR_R2, x, r.data() + 4 * i);
        const uint64_t m = class_m[cls[i]];
        ks.push_back(i % 3 == 0 ? m - 1 : i % 3 == 1 ? 0 : rnd() % m);
        rows.push_back(M == 1 ? 0 : rnd() % M);
    }
    MixedPlan p;
    mixed_plan(c.n.data(), c.l.data(), S, cls.data(), N, &p);
    coset_batch_scalars_mixed(class_m.data(), S, cls.data(), ks.data(), rows.data(), r.data(), p.perm.data(), N, M, out.data(), threads_for);
    std::vector<uint64_t> row_w(4 * M, 0);
    for (size_t j = 0; j < N; ++j) {
        const size_t i = p.perm[j];
        const uint64_t s = cls[i];
        uint64_t h[4], want[4];
        fr_pow(fr_roots().w[__builtin_ctzll(c.n[s])], ks[i] * c.l[s], h);                     // w_s^(k l_s), the slow way
        fr_mul(r.data() + 4 * i, h, want);
        for (int q = 0; q < 4; ++q) {
            CHECK(out[4 * j + q] == r[4 * i + q], "case %d slot %zu: r", tag, j);
            CHECK(out[4 * (N + j) + q] == want[q], "case %d slot %zu: shifted weight", tag, j);
        }
        fr_add(row_w.data() + 4 * rows[i], r.data() + 4 * i, row_w.data() + 4 * rows[i]);
    }
    for (size_t q = 0; q < 4 * M; ++q) CHECK(out[8 * N + q] == row_w[q], "case %d row word %zu", tag, q);
}

static void check_error_order() {
    const uint64_t n_ok[3] = {64, 1024, 256}, l_ok[3] = {16, 16, 4};
    const uint64_t si[4] = {0, 1, 2, 1}, ki[4] = {3, 63, 0, 5}, ci[4] = {0, 1, 1, 0};
    std::vector<uint64_t> g2(48, 7);
    size_t l_max = 0, total = 0;
    auto run = [&](bool bad, const uint64_t* n, const uint64_t* l, size_t S, size_t srs_len, size_t M, const uint64_t* c, const uint64_t* s, const uint64_t* k, size_t count,
                   const uint64_t* g) { return mixed_checks(bad, n, l, S, srs_len, M, c, s, k, count, g, &l_max, &total); };
    CHECK(run(false, n_ok, l_ok, 3, 16, 2, ci, si, ki, 4, g2.data()) == KZG_OK && l_max == 16 && total == 16 + 16 + 4 + 16, "valid");
    CHECK(run(false, n_ok, l_ok, 3, 16, 2, ci, si, ki, 0, g2.data()) == KZG_OK && total == 0, "count = 0");
    CHECK(run(false, nullptr, nullptr, 0, 16, 2, ci, si, ki, 0, nullptr) == KZG_OK && l_max == 0, "nothing at all");
    // 1 before everything
    const uint64_t n_bad[3] = {64, 96, 256};
    CHECK(run(true, n_bad, l_ok, 600, 1, 2, ci, si, ki, 4, g2.data()) == KZG_ERR_INVALID_ARG, "1");
    // 2: no class, items
    CHECK(run(false, n_ok, l_ok, 0, 16, 2, ci, si, ki, 4, g2.data()) == KZG_ERR_INVALID_ARG, "2");
    // 3 before 4: 513 classes, the second of them broken
    std::vector<uint64_t> many_n(513, 64), many_l(513, 16);
    many_n[1] = 96;
    CHECK(run(false, many_n.data(), many_l.data(), 513, 16, 2, ci, si, ki, 4, nullptr) == KZG_ERR_TOO_LARGE, "3");
    CHECK(run(false, many_n.data(), many_l.data(), 512, 16, 2, ci, si, ki, 4, nullptr) == KZG_ERR_NOT_POWER_OF_TWO, "4 at 512 classes");
    // 4: in class order, coset_domain_check's own codes, before the SRS
    const uint64_t n_dom[3] = {64, (uint64_t)1 << 25, 96}, l_3[3] = {16, 3, 4}, l_big[3] = {16, 16, 256}, n_one[3] = {64, 1, 256};
    CHECK(run(false, n_bad, l_ok, 3, 1, 2, ci, si, ki, 4, g2.data()) == KZG_ERR_NOT_POWER_OF_TWO, "4a");
    CHECK(run(false, n_dom, l_3, 3, 1, 2, ci, si, ki, 4, g2.data()) == KZG_ERR_DOMAIN, "4b: class 1 before class 2, the domain before the chunk");
    CHECK(run(false, n_ok, l_3, 3, 1, 2, ci, si, ki, 4, g2.data()) == KZG_ERR_INVALID_ARG, "4c");
    CHECK(run(false, n_ok, l_big, 3, 1, 2, ci, si, ki, 4, g2.data()) == KZG_ERR_INVALID_ARG, "4d: l = n");
    CHECK(run(false, n_one, l_ok, 3, 1, 2, ci, si, ki, 4, g2.data()) == KZG_ERR_INVALID_ARG, "4e: n = 1");
    // 5 before 6: an EMPTY class counts for l_max
    const uint64_t l_wide[3] = {16, 16, 128}, s_two[4] = {0, 1, 0, 1}, k_bad[4] = {3, 64, 0, 5}, s_bad[4] = {0, 3, 2, 1}, c_bad[4] = {0, 2, 1, 0};
    CHECK(run(false, n_ok, l_wide, 3, 64, 2, ci, s_two, k_bad, 4, nullptr) == KZG_ERR_SRS_CAPACITY_EXCEEDED, "5");
    CHECK(run(false, n_ok, l_wide, 3, 128, 2, ci, s_two, k_bad, 4, nullptr) == KZG_ERR_INVALID_ARG, "6 behind 5");
    // 6
    CHECK(run(false, n_ok, l_ok, 3, 16, 2, ci, s_bad, ki, 4, g2.data()) == KZG_ERR_INVALID_ARG, "6a");
    const uint64_t k_m[4] = {4, 63, 0, 5};                                                    // m of class 0 is 4
    CHECK(run(false, n_ok, l_ok, 3, 16, 2, ci, si, k_m, 4, g2.data()) == KZG_ERR_INVALID_ARG, "6b");
    CHECK(run(false, n_ok, l_ok, 3, 16, 2, c_bad, si, ki, 4, g2.data()) == KZG_ERR_INVALID_ARG, "6c");
    CHECK(run(false, n_ok, l_ok, 3, 16, 2, nullptr, si, ki, 4, nullptr) == KZG_OK, "no commitments in this entry");
    // 7 before 8: 2^28 / 2^22 + 1 items of l = 2^22; the G2 points of classes 0 and 1 differ
    const uint64_t n_huge[2] = {(uint64_t)1 << 23, (uint64_t)1 << 24}, l_huge[2] = {(uint64_t)1 << 22, (uint64_t)1 << 22};
    std::vector<uint64_t> zeros(65, 0), g2d(32, 7);
    g2d[16] = 8;
    CHECK(run(false, n_huge, l_huge, 2, (size_t)1 << 22, 1, zeros.data(), zeros.data(), zeros.data(), 65, g2d.data()) == KZG_ERR_TOO_LARGE, "7");
    CHECK(run(false, n_huge, l_huge, 2, (size_t)1 << 22, 1, zeros.data(), zeros.data(), zeros.data(), 64, g2d.data()) == KZG_ERR_INVALID_ARG, "8 behind 7");
    // 8: classes 0 and 1 share l = 16; class 2 may carry anything
    std::vector<uint64_t> g2e(48, 7);
    g2e[47] = 9;
    CHECK(run(false, n_ok, l_ok, 3, 16, 2, ci, si, ki, 4, g2e.data()) == KZG_OK, "8: another length");
    g2e[31] = 9;
    CHECK(run(false, n_ok, l_ok, 3, 16, 2, ci, si, ki, 4, g2e.data()) == KZG_ERR_INVALID_ARG, "8");
    CHECK(run(false, n_ok, l_ok, 3, 16, 2, ci, si, ki, 0, g2e.data()) == KZG_ERR_INVALID_ARG, "8 with no items: all classes are compared");
}

int main() {
    std::vector<Case> grid = {
        {{2}, {1}, {1}},
        {{2, 32, 32, 4096, 16384, 4096, 2048, 4096, 8192, (uint64_t)1 << 24, 256}, {1, 1, 16, 16, 16, 64, 512, 1024, 2048, 16, 4}, {2, 513, 33, 31, 3, 9, 2, 2, 1, 2, 0}},
        {{64, 64, 64}, {16, 16, 16}, {5, 0, 7}},                                              // repeated classes, one of them empty
        {{256, 64}, {4, 16}, {0, 0}},                                                         // nothing at all
        {{4096, 8192}, {2048, 4096}, {3, 2}},                                                 // only the per-coset route
        {{1024, 4096}, {1, 1024}, {600000, 700}},                                             // more tiles than workgroups in both launches
        {{65536, 16384}, {64, 16}, {32768, 32768}},
        {{2048}, {1024}, {5000}},
    };
    {   // 512 classes of every tiled length, more tiles than workgroups: every class still gets one
        Case c;
        for (int s = 0; s < 512; ++s) { c.n.push_back(4096); c.l.push_back((uint64_t)1 << (s % 11)); c.counts.push_back(s % 7 == 3 ? 0 : 1 + (uint64_t)(rnd() % 3000)); }
        grid.push_back(c);
    }
    {   // 512 classes, one item each
        Case c;
        for (int s = 0; s < 512; ++s) { c.n.push_back((uint64_t)1 << (12 + s % 3)); c.l.push_back((uint64_t)1 << (s % 12)); c.counts.push_back(1); }
        grid.push_back(c);
    }
    for (size_t g = 0; g < grid.size(); ++g) check_plan(grid[g], (int)g);
    for (size_t g = 0; g < grid.size(); ++g) {
        size_t N = 0;
        for (uint64_t v : grid[g].counts) N += v;
        if (N <= 5000) { check_scalars(grid[g], 1, (int)g); check_scalars(grid[g], 5, (int)g); }
    }
    check_scalars(Case{{(uint64_t)1 << 24, 4}, {1, 2}, {1030, 3}}, 2000, 100);                   // m = 2^24 beside m = 2; M > N; 32 chunks
    check_error_order();
    printf("ok %zu\n", checks);
    return 0;
}
