// locatecheck.cpp -- csrc/host_locate.h as a plain host program (g++, also with -fsanitize=address,undefined; no GPU, no library): the
// group checks, the counting-sort plan against a naive stable sort, the search over a fake predicate with planted bad groups (located set
// and the bound on predicate calls), and the search with the real host pairing on points built with host_curve.h / host_pairing.h.
// Prints "locatecheck ok"; a failed check prints its line and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <set>
#include <vector>

#include "host_locate.h"
#include "host_pairing.h"

using namespace kzg;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "locatecheck: line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)

// ---- the plan ------------------------------------------------------------------------------------------------------------------------
static void check_plan(const std::vector<uint64_t>& gi, size_t n_groups) {
    const size_t count = gi.size();
    CHECK(locate_check_groups(gi.data(), count, n_groups) == KZG_OK);
    LocatePlan p;
    CHECK(locate_plan(gi.data(), count, n_groups, &p) == KZG_OK);
    CHECK(p.count == count && p.n_groups == n_groups && p.perm.size() == count && p.offsets.size() == n_groups + 1 && p.seg_of.size() == count);
    std::vector<uint32_t> naive(count);
    std::iota(naive.begin(), naive.end(), 0u);
    std::stable_sort(naive.begin(), naive.end(), [&](uint32_t a, uint32_t b) { return gi[a] < gi[b]; });
    CHECK(naive == p.perm);
    CHECK(p.offsets[0] == 0 && p.offsets[n_groups] == count);
    for (size_t g = 0; g < n_groups; ++g) {
        CHECK(p.offsets[g] <= p.offsets[g + 1]);
        for (uint32_t s = p.offsets[g]; s < p.offsets[g + 1]; ++s) CHECK(gi[p.perm[s]] == g);
    }
    // the non-empty groups, their offsets, the segment of every sorted position
    std::vector<uint32_t> segs;
    for (size_t g = 0; g < n_groups; ++g) if (p.offsets[g] != p.offsets[g + 1]) segs.push_back((uint32_t)g);
    CHECK(segs == p.segs && p.seg_off.size() == segs.size() + 1 && p.part_off.size() == segs.size() + 1 && p.seg_off[0] == 0 && p.part_off[0] == 0);
    std::set<std::pair<uint32_t, uint32_t>> pieces;                                  // (wave, segment) pairs that hold an item
    for (size_t j = 0; j < segs.size(); ++j) {
        CHECK(p.seg_off[j] == p.offsets[segs[j]] && p.seg_off[j + 1] == p.offsets[segs[j] + 1]);
        for (uint32_t s = p.seg_off[j]; s < p.seg_off[j + 1]; ++s) { CHECK(p.seg_of[s] == j); pieces.insert({s / LOCATE_WAVE, (uint32_t)j}); }
    }
    CHECK(p.part_off.back() == pieces.size());
    std::set<uint32_t> slots;                                                        // every piece has a slot of its own inside its segment's range
    for (const auto& pc : pieces) {
        const uint32_t j = pc.second, slot = p.part_off[j] + pc.first - p.seg_off[j] / LOCATE_WAVE;
        CHECK(slot >= p.part_off[j] && slot < p.part_off[j + 1]);
        CHECK(slots.insert(slot).second);
    }
}

static void plans() {
    for (size_t G : {1, 2, 3, 64, 65, 1000}) {
        std::vector<uint64_t> gi;
        gi.assign(3 * G + 1, 0);                                                     // everything in one group (the others empty)
        check_plan(gi, G);
        gi.assign(130, G - 1);
        check_plan(gi, G);
        gi.resize(G);                                                                // one group per item
        std::iota(gi.begin(), gi.end(), (uint64_t)0);
        check_plan(gi, G);
        std::reverse(gi.begin(), gi.end());
        check_plan(gi, G);
        gi.resize(3 * G + 1);                                                        // interleaved
        for (size_t i = 0; i < gi.size(); ++i) gi[i] = i % G;
        check_plan(gi, G);
        gi.resize(257);                                                              // with empty groups: every third group only
        for (size_t i = 0; i < gi.size(); ++i) gi[i] = (i * 7 % G) / 3 * 3;
        check_plan(gi, G);
        if (G >= 3) {                                                                // the first and the last group empty
            gi.resize(2 * G + 63);
            for (size_t i = 0; i < gi.size(); ++i) gi[i] = 1 + (i * 5) % (G - 2);
            check_plan(gi, G);
        }
        check_plan({}, G);                                                           // no items: every group empty
    }
    check_plan({}, 0);
    // segments that end at the wave and workgroup edges 63|64 and 255|256, and one that crosses both
    {
        std::vector<uint64_t> gi(300);
        for (size_t i = 0; i < 300; ++i) gi[i] = i < 64 ? 0 : i < 256 ? 1 : 2;
        check_plan(gi, 3);
        for (size_t i = 0; i < 300; ++i) gi[i] = i < 10 ? 0 : i < 290 ? 1 : 2;
        check_plan(gi, 3);
    }
    const uint64_t at[2] = {0, 3};
    LocatePlan p;
    CHECK(locate_check_groups(at, 2, 3) == KZG_ERR_INVALID_ARG);                     // a group index = n_groups
    CHECK(locate_check_groups(at, 2, 4) == KZG_OK);
    CHECK(locate_check_groups(at, 1, 0) == KZG_ERR_INVALID_ARG);                     // n_groups = 0 with count > 0
    CHECK(locate_check_groups(at, 0, 0) == KZG_OK);
    CHECK(locate_plan(at, 0, LOCATE_MAX_GROUPS + 1, &p) == KZG_ERR_TOO_LARGE && p.offsets.empty());   // before anything is allocated
}

// ---- the search over a fake predicate: a "point" is the number of bad groups in the range --------------------------------------------
struct CountOps {
    long zero() const { return 0; }
    long add(long a, long b) const { return a + b; }
    long sub(long a, long b) const { return a - b; }
};
static void search_case(size_t G, const std::set<size_t>& bad) {
    std::vector<long> lhs(G, 0), rhs(G, 0);
    for (size_t g : bad) { lhs[g] = 1; rhs[g] = 1; }
    std::vector<uint8_t> ok(G, 7);
    size_t n_bad = 99, seen = 0;
    auto holds = [&](long l, long r) { ++seen; CHECK(l == r && l >= 0); return l == 0; };
    const size_t calls = locate_search(lhs.data(), rhs.data(), G, CountOps(), holds, ok.data(), &n_bad);
    CHECK(calls == seen && n_bad == bad.size());
    for (size_t g = 0; g < G; ++g) CHECK(ok[g] == (bad.count(g) ? 0 : 1));
    CHECK(calls <= locate_max_checks(G, bad.size()));
    if (bad.empty()) CHECK(calls == 1);                                              // the good batch: the root alone
}
static void searches() {
    CHECK(locate_max_checks(1, 1) == 1 && locate_max_checks(2, 1) == 3 && locate_max_checks(33, 2) == 25 && locate_max_checks(8, 0) == 1);
    for (size_t G : {1, 2, 3, 5, 8, 33}) {
        search_case(G, {});
        for (size_t a = 0; a < G; ++a) {
            search_case(G, {a});
            for (size_t b = a + 1; b < G; ++b) search_case(G, {a, b});
        }
        std::set<size_t> all;
        for (size_t g = 0; g < G; ++g) all.insert(g);
        search_case(G, all);
    }
    size_t n_bad = 5;
    CHECK(locate_search((const long*)nullptr, (const long*)nullptr, 0, CountOps(), [](long, long) { return true; }, (uint8_t*)nullptr, &n_bad) == 0 && n_bad == 0);
}

// ---- the search with the real pairing: L_g = [s_g] G1, R_g = [s_g x] G1 against "[tau^l]_2" = [x] G2, one pair broken ------------------
namespace H = kzg_host;
struct CurveOps {
    H::Xyzz zero() const { return H::xyzz_inf(); }
    H::Xyzz add(const H::Xyzz& a, const H::Xyzz& b) const { return H::xyzz_add(a, b); }
    H::Xyzz sub(const H::Xyzz& a, H::Xyzz b) const { b.y = H::neg(b.y); return H::xyzz_add(a, b); }
};
static H::Xyzz leaf(uint64_t k) {
    const uint64_t kw[4] = {k, 0, 0, 0};
    uint64_t xy[8];
    H::g1_to_wire(H::g1_mul_generator(kw), xy);
    return H::xyzz_from_affine_wire(xy);
}
static void pairing_search() {
    const uint64_t x = 0x9e377, xw[4] = {x, 0, 0, 0};
    const H::G2 g2x = H::g2_mul_generator(xw), g2 = H::g2_generator();
    const size_t G = 6;
    const uint64_t s[G] = {3, 1000003, 0, 77, 77, 12345};                            // a zero pair (the identity twice) and two equal pairs
    for (int broken = -1; broken < (int)G; broken += 3) {                            // none, group 2, group 5
        std::vector<H::Xyzz> lhs, rhs;
        for (size_t g = 0; g < G; ++g) { lhs.push_back(leaf(s[g])); rhs.push_back(leaf(s[g] * x + ((int)g == broken ? 1 : 0))); }
        auto holds = [&](const H::Xyzz& l, const H::Xyzz& r) {
            uint64_t a[8], b[8];
            H::xyzz_to_affine(l, a, nullptr);
            H::xyzz_to_affine(r, b, nullptr);
            return H::pairings_verify(H::g1_from_wire(a), g2x, H::g1_from_wire(b), g2);
        };
        std::vector<uint8_t> ok(G, 7);
        size_t n_bad = 0;
        const size_t calls = locate_search(lhs.data(), rhs.data(), G, CurveOps(), holds, ok.data(), &n_bad);
        CHECK(n_bad == (broken < 0 ? 0u : 1u) && calls <= locate_max_checks(G, n_bad) && (broken >= 0 || calls == 1));
        for (size_t g = 0; g < G; ++g) CHECK(ok[g] == ((int)g == broken ? 0 : 1));
    }
}

int main() {
    plans();
    searches();
    pairing_search();
    printf("locatecheck ok\n");
    return 0;
}
