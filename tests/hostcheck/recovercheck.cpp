// recovercheck.cpp -- csrc/host_recover.h as a plain host program (g++ -fsanitize=address,undefined, no GPU, no library): every error of
// the documented table in its order, the list of missing cosets and the item map for full, partial and refused inputs, and the cost cap
// at its edge.  Prints "recovercheck ok"; a failed check prints its line and exits 1.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "host_recover.h"

using namespace kzg;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "recovercheck: line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)

static int32_t plan_of(const std::vector<uint64_t>& ks, size_t n, size_t l, size_t bound, RecoverPlan* p, bool any_null = false) {
    return recover_plan(any_null, ks.data(), ks.size(), n, l, bound, p);
}
static bool empty(const RecoverPlan& p) { return p.n == 0 && p.m == 0 && p.missing.empty() && p.item_of.empty(); }

int main() {
    RecoverPlan p;
    // ---- the error table, each case wrong in its own check AND in every later one that can be wrong at the same time: the earlier wins
    const std::vector<uint64_t> dup = {1, 1}, high = {0, 4}, two = {0, 1};
    CHECK(plan_of(dup, 0, 3, 99, &p, true) == KZG_ERR_INVALID_ARG && empty(p));               // 1. null pointer, in front of a bad n
    CHECK(plan_of(dup, 0, 3, 99, &p) == KZG_ERR_NOT_POWER_OF_TWO && empty(p));                // 2. n = 0
    CHECK(plan_of(dup, 24, 3, 99, &p) == KZG_ERR_NOT_POWER_OF_TWO);                           //    n not a power of two
    CHECK(plan_of(dup, (size_t)1 << 25, 3, 99, &p) == KZG_ERR_DOMAIN);                        // 3. n > 2^24, in front of a bad chunk length
    CHECK(plan_of(dup, 1, 1, 99, &p) == KZG_ERR_INVALID_ARG);                                 // 4. n = 1
    CHECK(plan_of(two, 16, 0, 0, &p) == KZG_ERR_INVALID_ARG);                                 //    l = 0
    CHECK(plan_of(two, 16, 3, 0, &p) == KZG_ERR_INVALID_ARG);                                 //    l not a power of two
    CHECK(plan_of(two, 16, 16, 0, &p) == KZG_ERR_INVALID_ARG);                                //    l > n / 2
    CHECK(plan_of({}, 16, 4, 0, &p) == KZG_ERR_INVALID_ARG && empty(p));                      // 5. count = 0 (the empty input)
    CHECK(plan_of({0, 1, 2, 3, 0}, 16, 4, 0, &p) == KZG_ERR_INVALID_ARG);                     //    count > m
    CHECK(plan_of(high, 16, 4, 0, &p) == KZG_ERR_INVALID_ARG && empty(p));                    // 6. an index = m
    CHECK(plan_of({0, ~(uint64_t)0}, 16, 4, 0, &p) == KZG_ERR_INVALID_ARG);                   //    an index far outside
    CHECK(plan_of(dup, 16, 4, 0, &p) == KZG_ERR_INVALID_ARG && empty(p));                     //    a duplicate
    CHECK(plan_of(two, 16, 4, 9, &p) == KZG_ERR_INVALID_ARG && empty(p));                     // 7. degree_bound = count l + 1
    CHECK(plan_of({0}, (size_t)1 << 24, 1, 2, &p) == KZG_ERR_INVALID_ARG);                    //    ... in front of the cap
    CHECK(plan_of({0}, (size_t)1 << 24, 1, 1, &p) == KZG_ERR_TOO_LARGE && empty(p));          // 8. the cap: m (m - 1) = 2^48 - 2^24
    // a duplicate is reported, not the cap it would also hit
    CHECK(plan_of({5, 5}, (size_t)1 << 24, 1, 0, &p) == KZG_ERR_INVALID_ARG);

    // ---- the plan: partial, full, one coset
    CHECK(plan_of({3, 0}, 16, 4, 0, &p) == KZG_OK);
    CHECK(p.n == 16 && p.l == 4 && p.m == 4 && p.count == 2 && p.log_n == 4 && p.log_l == 2 && p.log_m == 2 && p.degree_bound == 8);
    CHECK((p.missing == std::vector<uint32_t>{1, 2}));
    CHECK((p.item_of == std::vector<uint32_t>{1, RECOVER_NO_ITEM, RECOVER_NO_ITEM, 0}));
    CHECK(plan_of({3, 0}, 16, 4, 5, &p) == KZG_OK && p.degree_bound == 5);
    CHECK(plan_of({2, 3, 1, 0}, 16, 4, 16, &p) == KZG_OK);                                    // every coset: nothing missing
    CHECK(p.missing.empty() && (p.item_of == std::vector<uint32_t>{3, 2, 0, 1}) && p.degree_bound == 16);
    CHECK(plan_of({1}, 2, 1, 0, &p) == KZG_OK && (p.missing == std::vector<uint32_t>{0}) && p.degree_bound == 1 && p.log_m == 1);
    CHECK(plan_of({0}, 2048, 1024, 0, &p) == KZG_OK && p.m == 2 && (p.missing == std::vector<uint32_t>{1}) && p.degree_bound == 1024);
    {   // every odd coset missing at m = 2^16: inside the cap whatever is missing
        std::vector<uint64_t> ks;
        for (uint64_t k = 0; k < 65536; k += 2) ks.push_back(k);
        CHECK(plan_of(ks, (size_t)1 << 20, 16, 0, &p) == KZG_OK && p.missing.size() == 32768 && p.missing[0] == 1 && p.missing.back() == 65535);
        CHECK(plan_of({7}, (size_t)1 << 16, 1, 0, &p) == KZG_OK && p.missing.size() == 65535);   // m (m - 1) < 2^32
    }

    // ---- the cap at its edge: m (m - count) = 2^32 passes, 2^32 + m does not
    {
        const size_t n = (size_t)1 << 20, m = n;                                              // l = 1: m - count = 2^12 <=> m (m - count) = 2^32
        std::vector<uint64_t> ks(m - 4096);
        std::iota(ks.begin(), ks.end(), (uint64_t)0);
        CHECK(plan_of(ks, n, 1, 0, &p) == KZG_OK && p.missing.size() == 4096 && p.missing[0] == m - 4096);
        ks.pop_back();                                                                        // m - count = 2^12 + 1
        CHECK(plan_of(ks, n, 1, 0, &p) == KZG_ERR_TOO_LARGE && empty(p));
    }
    {
        const size_t n = (size_t)1 << 24, l = 2, m = n / l;                                   // m = 2^23: m - count = 2^9
        std::vector<uint64_t> ks(m - 512);
        std::iota(ks.begin(), ks.end(), (uint64_t)512);
        CHECK(plan_of(ks, n, l, 0, &p) == KZG_OK && p.missing.size() == 512 && p.missing.back() == 511);
        ks.pop_back();
        CHECK(plan_of(ks, n, l, 0, &p) == KZG_ERR_TOO_LARGE);
    }
    printf("recovercheck ok\n");
    return 0;
}
