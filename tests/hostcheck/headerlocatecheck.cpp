// headerlocatecheck.cpp -- csrc/host_header_locate.h as a plain host program (g++, also with -fsanitize=address,undefined; no GPU, no
// library): the composite keys and the plan of the 2 count G2 points against a naive grouping, the assembly of segment sums into
// per-group components, the error table in its order, and the search for planted bad groups with its bound on the checks.
//
// The stand-in group: G1, G2 and the pairing's target are the integers modulo the prime Q = 2^61 - 1, a point [a]G is the number a, and
// e([a]G1, [b]G2) is a b, so "the product of the pairings is one" reads "the sum of the products is zero".  Headers are made as the
// GPU test makes them: C = f, C2 = f, pi2 = tau^(N - d) f for a scalar f.
// Prints "headerlocatecheck ok"; a failed check prints its line and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "host_header_locate.h"

using namespace kzg;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "headerlocatecheck: line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)

static const uint64_t Q = ((uint64_t)1 << 61) - 1;
static uint64_t madd(uint64_t a, uint64_t b) { return (a + b) % Q; }
static uint64_t msub(uint64_t a, uint64_t b) { return (a + Q - b) % Q; }
static uint64_t mmul(uint64_t a, uint64_t b) { return (uint64_t)((unsigned __int128)a * b % Q); }
static uint64_t mpow(uint64_t a, uint64_t e) { uint64_t r = 1; for (; e; e >>= 1, a = mmul(a, a)) if (e & 1) r = mmul(r, a); return r; }
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

struct ModOps {
    uint64_t zero() const { return 0; }
    uint64_t add(uint64_t a, uint64_t b) const { return madd(a, b); }
    uint64_t sub(uint64_t a, uint64_t b) const { return msub(a, b); }
};
using Sums = HeaderSums<uint64_t, uint64_t>;
using Ops = HeaderSumOps<uint64_t, uint64_t, ModOps, ModOps>;

// ---- a batch in the stand-in group ---------------------------------------------------------------------------------------------------
struct Batch {
    size_t count = 0, n_groups = 0, n_shifts = 0;
    uint64_t tau = 0, rho = 0, order = 1024;
    std::vector<uint64_t> shift_lens, T;                 // T_s = tau^(N - shift_lens[s])
    std::vector<uint64_t> lens, gi, r, c, c2, pi2;
    std::vector<uint8_t> cls;
};
static Batch make_batch(size_t count, size_t n_groups, const std::vector<uint64_t>& shift_lens, const std::vector<size_t>& class_cycle) {
    Batch b;
    b.count = count; b.n_groups = n_groups; b.n_shifts = shift_lens.size(); b.shift_lens = shift_lens;
    b.tau = rnd() % Q; b.rho = rnd() % Q;
    for (uint64_t d : shift_lens) b.T.push_back(mpow(b.tau, b.order - d));
    for (size_t i = 0; i < count; ++i) {
        const size_t s = class_cycle[i % class_cycle.size()];
        const uint64_t f = rnd() % Q;
        b.lens.push_back(shift_lens[s]);
        b.gi.push_back(n_groups ? rnd() % n_groups : 0);
        b.r.push_back(rnd() % Q);
        b.c.push_back(f); b.c2.push_back(f); b.pi2.push_back(mmul(b.T[s], f));
    }
    return b;
}
static void classify(Batch& b) {
    HeaderGrouping grp;
    grp.on = true; grp.group_indices = b.gi.data(); grp.n_groups = b.n_groups;
    CHECK(header_batch_checks(false, b.c.data(), b.c2.data(), b.pi2.data(), b.lens.data(), b.count, b.shift_lens.data(), b.T.data(), b.n_shifts, grp, &b.cls, nullptr) == KZG_OK);
    CHECK(b.cls.size() == b.count);
    for (size_t i = 0; i < b.count; ++i) CHECK(b.shift_lens[b.cls[i]] == b.lens[i]);
}

// ---- keys and the plan against a naive grouping ----------------------------------------------------------------------------------------
struct Planned {
    LocatePlan g1, g2;
    HeaderClasses cls;
    std::vector<Sums> lhs, rhs;
};
static Planned plan_and_assemble(Batch& b) {
    classify(b);
    Planned p;
    std::vector<uint64_t> keys;
    header_locate_keys(b.gi.data(), b.cls.data(), b.count, b.n_groups, b.n_shifts, &keys);
    CHECK(keys.size() == 2 * b.count);
    const size_t n_keys = header_n_keys(b.n_groups, b.n_shifts);
    CHECK(n_keys == b.n_groups * b.n_shifts + b.n_groups);
    std::map<uint64_t, std::vector<uint32_t>> naive;     // key -> its points, ascending (the caller's order)
    for (size_t i = 0; i < b.count; ++i) {
        CHECK(keys[2 * i] == b.gi[i] * b.n_shifts + b.cls[i] && keys[2 * i] < b.n_groups * b.n_shifts);
        CHECK(keys[2 * i + 1] == b.n_groups * b.n_shifts + b.gi[i] && keys[2 * i + 1] < n_keys);
        naive[keys[2 * i]].push_back((uint32_t)(2 * i));
        naive[keys[2 * i + 1]].push_back((uint32_t)(2 * i + 1));
    }
    CHECK(locate_check_groups(keys.data(), keys.size(), n_keys) == KZG_OK);
    CHECK(locate_plan(keys.data(), keys.size(), n_keys, &p.g2) == KZG_OK);
    CHECK(p.g2.count == 2 * b.count && p.g2.segs.size() == naive.size());
    size_t j = 0;
    for (const auto& kv : naive) {                       // ascending keys: the order of the segments
        CHECK(p.g2.segs[j] == kv.first);
        CHECK(p.g2.seg_off[j + 1] - p.g2.seg_off[j] == kv.second.size());
        for (size_t t = 0; t < kv.second.size(); ++t) { CHECK(p.g2.perm[p.g2.seg_off[j] + t] == kv.second[t]); CHECK(p.g2.seg_of[p.g2.seg_off[j] + t] == j); }
        ++j;
    }
    // every piece a wave leaves has a slot of its own below part_off.back(): the bound of the device's stores
    std::set<uint32_t> slots;
    for (uint32_t s = 0; s < p.g2.count; ++s) {
        const uint32_t seg = p.g2.seg_of[s];
        if (s % LOCATE_WAVE != 0 && p.g2.seg_of[s - 1] == seg) continue;
        const uint32_t slot = p.g2.part_off[seg] + s / LOCATE_WAVE - p.g2.seg_off[seg] / LOCATE_WAVE;
        CHECK(slot >= p.g2.part_off[seg] && slot < p.g2.part_off[seg + 1] && p.g2.part_off[seg + 1] <= p.g2.part_off.back());
        CHECK(slots.insert(slot).second);
    }
    CHECK(slots.size() == p.g2.part_off.back());
    CHECK(locate_plan(b.gi.data(), b.count, b.n_groups, &p.g1) == KZG_OK);
    // the segment sums the device would leave, through the plans
    std::vector<uint64_t> seg_u(p.g1.segs.size(), 0), seg_q(p.g2.segs.size(), 0);
    for (size_t s = 0; s < p.g1.segs.size(); ++s)
        for (uint32_t t = p.g1.seg_off[s]; t < p.g1.seg_off[s + 1]; ++t) seg_u[s] = madd(seg_u[s], mmul(b.r[p.g1.perm[t]], b.c[p.g1.perm[t]]));
    for (size_t s = 0; s < p.g2.segs.size(); ++s)
        for (uint32_t t = p.g2.seg_off[s]; t < p.g2.seg_off[s + 1]; ++t) {
            const uint32_t pt = p.g2.perm[t];
            seg_q[s] = madd(seg_q[s], mmul(b.r[pt >> 1], pt & 1 ? b.pi2[pt >> 1] : b.c2[pt >> 1]));
        }
    p.cls = header_present_classes(b.cls.data(), b.count, b.n_shifts);
    header_assemble(p.g1, p.g2, b.n_groups, b.n_shifts, p.cls, [&](size_t s) { return seg_u[s]; }, [&](size_t s) { return seg_q[s]; }, (uint64_t)0, (uint64_t)0, &p.lhs,
                    &p.rhs);
    return p;
}

static void check_components(Batch& b) {
    const Planned p = plan_and_assemble(b);
    // the classes present, ascending, and nothing sized by the 64-entry maximum
    std::set<uint32_t> present(b.cls.begin(), b.cls.end());
    CHECK(std::vector<uint32_t>(present.begin(), present.end()) == p.cls.present && p.cls.slot_of.size() == b.n_shifts);
    for (size_t s = 0; s < b.n_shifts; ++s) CHECK(present.count((uint32_t)s) ? p.cls.present[p.cls.slot_of[s]] == s : p.cls.slot_of[s] == -1);
    CHECK(p.lhs.size() == b.n_groups && p.rhs.size() == b.n_groups);
    for (size_t g = 0; g < b.n_groups; ++g) {
        uint64_t u = 0, pi = 0;
        std::vector<uint64_t> w(b.n_shifts, 0);
        for (size_t i = 0; i < b.count; ++i) {
            if (b.gi[i] != g) continue;
            u = madd(u, mmul(b.r[i], b.c[i]));
            pi = madd(pi, mmul(b.r[i], b.pi2[i]));
            w[b.cls[i]] = madd(w[b.cls[i]], mmul(b.r[i], b.c2[i]));
        }
        CHECK(p.lhs[g].u == u && p.lhs[g].q.empty());
        CHECK(p.rhs[g].u == 0 && p.rhs[g].q.size() == 1 + present.size() && p.rhs[g].q[0] == pi);
        for (size_t c = 0; c < p.cls.present.size(); ++c) CHECK(p.rhs[g].q[1 + c] == w[p.cls.present[c]]);
        for (size_t s = 0; s < b.n_shifts; ++s) if (!present.count((uint32_t)s)) CHECK(w[s] == 0);
    }
}

static void plans_and_components() {
    const std::vector<uint64_t> three = {1, 4, 1024};
    for (size_t count : {1, 2, 63, 64, 65, 257}) {
        for (size_t G : {(size_t)1, (size_t)3, count, count + 2}) {
            Batch b = make_batch(count, G, three, {1});                         // one class: the C2 and pi2 segments of a group are as long
            check_components(b);
            b = make_batch(count, G, three, {0, 1, 2});                         // alternating classes
            check_components(b);
            b = make_batch(count, G, {8, 1, 4, 1024, 2}, {3, 3, 1});            // two of five classes present
            check_components(b);
        }
        Batch b = make_batch(count, count, three, {0, 2});                      // "item": one group per header, in order
        for (size_t i = 0; i < count; ++i) b.gi[i] = i;
        check_components(b);
        for (size_t i = 0; i < count; ++i) b.gi[i] = count - 1 - i;
        check_components(b);
    }
    Batch b = make_batch(0, 4, three, {0});                                     // no header: every group the identity
    check_components(b);
    b = make_batch(0, 0, three, {0});
    check_components(b);
}

// ---- the error table, in its order ---------------------------------------------------------------------------------------------------------
static void errors() {
    const uint64_t sl[3] = {1, 4, 1024}, lens[4] = {4, 1, 4, 1024}, gi[4] = {0, 2, 1, 2};
    const uint64_t pts[4] = {1, 2, 3, 4};                                        // never read: pointers only
    std::vector<uint8_t> cls;
    uint64_t bad = 99;
    HeaderGrouping grp;
    grp.on = true; grp.group_indices = gi; grp.n_groups = 3;
    auto run = [&](bool handle_null, const void* c, const uint64_t* l, size_t count, const uint64_t* s, size_t n_shifts, const HeaderGrouping& g) {
        bad = 99;
        return header_batch_checks(handle_null, c, pts, pts, l, count, s, pts, n_shifts, g, &cls, &bad);
    };
    CHECK(run(false, pts, lens, 4, sl, 3, grp) == KZG_OK && cls == std::vector<uint8_t>({1, 0, 1, 2}) && bad == 99);
    CHECK(run(false, pts, lens, 4, sl, 3, HeaderGrouping()) == KZG_OK);          // the plain batch entry: no group rows
    // row 1 in front of everything: with a length that is no power of two, a bad group index and too many groups behind it
    const uint64_t odd[4] = {4, 6, 2, 1024};
    HeaderGrouping worst = grp;
    worst.n_groups = 2;
    CHECK(run(true, pts, odd, 4, sl, 3, worst) == KZG_ERR_INVALID_ARG);
    CHECK(run(false, nullptr, odd, 4, sl, 3, worst) == KZG_ERR_INVALID_ARG);
    CHECK(run(false, pts, nullptr, 4, sl, 3, worst) == KZG_ERR_INVALID_ARG);
    CHECK(run(false, pts, odd, 4, nullptr, 3, worst) == KZG_ERR_INVALID_ARG);
    CHECK(run(false, pts, odd, 4, sl, 0, worst) == KZG_ERR_INVALID_ARG);
    HeaderGrouping no_gi = worst;
    no_gi.group_indices = nullptr;
    CHECK(run(false, pts, odd, 4, sl, 3, no_gi) == KZG_ERR_INVALID_ARG);         // a null group_indices is a null pointer of row 1
    CHECK(run(false, pts, lens, 0, sl, 3, no_gi) == KZG_OK);                     // ... with count > 0 only
    std::vector<uint64_t> many(65);
    for (size_t k = 0; k < 65; ++k) many[k] = 3 * (k + 1);                       // 65 shifts, none a power of two: row 1 in front of row 2
    CHECK(run(false, pts, odd, 4, many.data(), 65, worst) == KZG_ERR_INVALID_ARG);
    const uint64_t dup[4] = {3, 4, 1024, 3};
    CHECK(run(false, pts, odd, 4, dup, 4, worst) == KZG_ERR_INVALID_ARG);        // a duplicate that is no power of two either
    // row 2 in front of rows 3, 4a
    const uint64_t sl_odd[3] = {1, 4, 1000};
    CHECK(run(false, pts, lens, 4, sl_odd, 3, worst) == KZG_ERR_NOT_POWER_OF_TWO);
    CHECK(run(false, pts, odd, 4, sl, 3, worst) == KZG_ERR_NOT_POWER_OF_TWO && bad == 99);      // 6 (row 2) in front of 2 (row 3)
    const uint64_t zero_len[4] = {4, 4, 0, 4};
    CHECK(run(false, pts, zero_len, 4, sl, 3, worst) == KZG_ERR_NOT_POWER_OF_TWO);
    // row 3 in front of row 4a, with the header's index
    const uint64_t unlisted[4] = {4, 1, 4, 2};
    CHECK(run(false, pts, unlisted, 4, sl, 3, worst) == KZG_ERR_INVALID_ARG && bad == 3);
    // row 4 in front of row 4a (the arrays are not read beyond the power-of-two rows: one shared length array)
    {
        const size_t big = HEADER_MAX_COUNT + 1;
        std::vector<uint64_t> l(big, 4), g(big, 7);
        HeaderGrouping gg;
        gg.on = true; gg.group_indices = g.data(); gg.n_groups = 3;
        CHECK(run(false, pts, l.data(), big, sl, 3, gg) == KZG_ERR_TOO_LARGE);
        CHECK(run(false, pts, l.data(), big - 1, sl, 3, gg) == KZG_ERR_INVALID_ARG && bad == 99);       // 4a: 7 >= 3
    }
    // row 4a in front of row 4b
    CHECK(run(false, pts, lens, 4, sl, 3, worst) == KZG_ERR_INVALID_ARG && bad == 99);          // group 2 of 2
    HeaderGrouping none = grp;
    none.n_groups = 0;
    CHECK(run(false, pts, lens, 4, sl, 3, none) == KZG_ERR_INVALID_ARG);         // n_groups = 0 with count > 0
    CHECK(run(false, pts, lens, 0, sl, 3, none) == KZG_OK && cls.empty());
    HeaderGrouping huge = grp;
    huge.n_groups = HEADER_MAX_KEYS / 4 + 1;                                     // (n_shifts + 1) n_groups just above 2^28
    CHECK(run(false, pts, lens, 4, sl, 3, huge) == KZG_ERR_TOO_LARGE);
    CHECK(run(false, pts, lens, 0, sl, 3, huge) == KZG_ERR_TOO_LARGE);           // whatever the count
    huge.n_groups = HEADER_MAX_KEYS / 4;
    CHECK(run(false, pts, lens, 4, sl, 3, huge) == KZG_OK);
    huge.n_groups = ~(size_t)0;                                                  // the product would wrap
    CHECK(run(false, pts, lens, 0, sl, 3, huge) == KZG_ERR_TOO_LARGE);
}

// ---- the search over planted bad groups -------------------------------------------------------------------------------------------------
static void search_case(size_t count, size_t G, const std::set<size_t>& bad_headers, int kind) {
    Batch b = make_batch(count, G, {1, 4, 1024}, {0, 1, 2, 1});
    if (G == count) for (size_t i = 0; i < count; ++i) b.gi[i] = i;
    std::set<size_t> bad_groups;
    for (size_t i : bad_headers) {
        bad_groups.insert(b.gi[i]);
        const uint64_t e = 1 + rnd() % (Q - 1);
        if (kind == 0) b.c[i] = madd(b.c[i], e);
        else if (kind == 1) b.c2[i] = madd(b.c2[i], e);
        else if (kind == 2) b.pi2[i] = madd(b.pi2[i], e);
        else b.lens[i] = b.lens[i] == 4 ? 1 : 4;                                 // another listed length: the proof is for the first
    }
    const Planned p = plan_and_assemble(b);
    HeaderFixed<uint64_t, uint64_t> fx;
    fx.g2 = 1; fx.neg_g1 = Q - 1; fx.neg_rho_g1 = msub(0, b.rho);
    for (uint32_t s : p.cls.present) fx.rho_shift.push_back(mmul(b.rho, b.T[s]));
    size_t seen = 0;
    auto holds = [&](const Sums& l, const Sums& r) {
        ++seen;
        CHECK(l.q.empty() && r.u == 0 && r.q.size() == 1 + p.cls.present.size());
        uint64_t sum_w = 0;
        for (size_t k = 1; k < r.q.size(); ++k) sum_w = madd(sum_w, r.q[k]);
        std::vector<uint64_t> ps, qs;
        header_pairs(fx, l.u, r.q, sum_w, &ps, &qs);
        CHECK(ps.size() == 3 + p.cls.present.size() && qs.size() == ps.size());
        uint64_t acc = 0;
        for (size_t k = 0; k < ps.size(); ++k) acc = madd(acc, mmul(ps[k], qs[k]));
        return acc == 0;
    };
    std::vector<uint8_t> ok(G, 7);
    size_t n_bad = 99;
    const size_t calls = locate_search(p.lhs.data(), p.rhs.data(), G, Ops(), holds, ok.data(), &n_bad);
    CHECK(calls == seen && n_bad == bad_groups.size());
    for (size_t g = 0; g < G; ++g) CHECK(ok[g] == (bad_groups.count(g) ? 0 : 1));
    CHECK(calls <= locate_max_checks(G, bad_groups.size()));
    if (bad_groups.empty()) CHECK(calls == 1);
}
static void searches() {
    for (int kind = 0; kind < 4; ++kind) {
        for (size_t count : {1, 2, 5, 65}) {
            search_case(count, count, {}, kind);
            for (size_t pos : {(size_t)0, count / 2, count - 1}) search_case(count, count, {pos}, kind);
            std::set<size_t> all;
            for (size_t i = 0; i < count; ++i) all.insert(i);
            search_case(count, count, all, kind);
        }
        search_case(257, 257, {100, 101, 256}, kind);                            // two adjacent
        search_case(257, 9, {3, 4, 200}, kind);                                  // random groups of about 28
        search_case(257, 1, {17}, kind);
        search_case(64, 80, {0, 63}, kind);                                      // more groups than headers: empty groups
    }
}

int main() {
    plans_and_components();
    errors();
    searches();
    printf("headerlocatecheck ok\n");
    return 0;
}
