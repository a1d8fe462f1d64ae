// tests/hostcheck/retrievetolerantcheck.cpp — TEST-ONLY stand-alone program: the pure host pieces of kzg_retrieve_blobs_bytes_tolerant and
// kzg_verify_multiproof_batch_locate_bytes (csrc/host_locate.h, csrc/host_recover.h).
//   1. locate_subset_plan against a brute-force plan: random subsets and groupings, segments that end at sorted positions 63 / 64 / 65, an
//      empty subset, a subset of one, and the grouping of the entry's second level (every chosen item a group of its own);
//   2. retrieve_choose: exactly use_count good items, use_count - 1, bad items first / last, every item bad;
//   3. recover_selected_plan against recover_batch_plan given the chosen cosets as its rows: patterns, missing lists, grouping and layout are
//      equal, the item map points into the HELD layout, a blob that is not recovered has no item, equal choices under one index row are one row;
//   4. the argument table of kzg_retrieve_blobs_bytes_tolerant (retrieve_tolerant_check) in its order, and the group rows of the located entry.
// Run by tests/test_retrieve_tolerant_host.py, once as it is and once under -fsanitize=address,undefined.  Prints "retrievetolerantcheck ok".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "host_locate.h"
#include "host_recover.h"

using namespace kzg;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (++failures <= 20) { fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static uint64_t rng_state = 0x13198A2E03707344ULL;
static uint64_t next64() {                         // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// ---- 1. the subset plan ---------------------------------------------------------------------------------------------------------------------
// brute force: the chosen items of every group in the order they were chosen; segments = the non-empty groups, ascending; the partial slots of
// a segment = the distinct waves of 64 sorted positions it touches
static void check_subset(const std::vector<uint32_t>& items, const std::vector<uint64_t>& groups, size_t n_groups, const char* what) {
    LocatePlan p;
    EXPECT(locate_subset_plan(items.data(), groups.data(), items.size(), n_groups, &p) == KZG_OK, "%s: refused", what);
    std::vector<uint32_t> perm, segs, seg_off(1, 0), seg_of, part_off(1, 0), offsets(1, 0);
    for (size_t g = 0; g < n_groups; ++g) {
        const size_t a = perm.size();
        for (size_t j = 0; j < items.size(); ++j) if (groups[j] == g) perm.push_back(items[j]);
        offsets.push_back((uint32_t)perm.size());
        if (perm.size() == a) continue;
        const uint32_t seg = (uint32_t)segs.size();
        segs.push_back((uint32_t)g);
        seg_off.push_back((uint32_t)perm.size());
        std::vector<uint32_t> waves;
        for (size_t s = a; s < perm.size(); ++s) { seg_of.push_back(seg); if (waves.empty() || waves.back() != s / 64) waves.push_back((uint32_t)(s / 64)); }
        part_off.push_back(part_off.back() + (uint32_t)waves.size());
    }
    EXPECT(p.count == items.size() && p.n_groups == n_groups, "%s: count / n_groups", what);
    EXPECT(p.perm == perm, "%s: perm", what);
    EXPECT(p.offsets == offsets, "%s: offsets", what);
    EXPECT(p.segs == segs && p.seg_off == seg_off && p.seg_of == seg_of, "%s: segments", what);
    EXPECT(p.part_off == part_off, "%s: partial slots", what);
    // what the kernels rely on: a lane's slot part_off[seg] + s / 64 - seg_off[seg] / 64 lies inside its segment's slots
    for (size_t s = 0; s < p.count; ++s) {
        const uint32_t j = p.seg_of[s], slot = p.part_off[j] + (uint32_t)(s / 64) - p.seg_off[j] / 64;
        EXPECT(slot >= p.part_off[j] && slot < p.part_off[j + 1], "%s: the slot of position %zu", what, s);
    }
}

static void check_subset_plans() {
    check_subset({}, {}, 0, "an empty subset, no group");
    check_subset({}, {}, 5, "an empty subset of five groups");
    check_subset({7}, {0}, 1, "a subset of one");
    check_subset({41}, {3}, 9, "a subset of one in group 3 of 9");
    for (size_t first : {63u, 64u, 65u}) {                                  // a first segment of 63 / 64 / 65 positions, singletons behind it, then a long one
        std::vector<uint32_t> items;
        std::vector<uint64_t> groups;
        for (size_t j = 0; j < first; ++j) { items.push_back((uint32_t)(1000 - 3 * j)); groups.push_back(0); }
        for (size_t j = 0; j < 5; ++j) { items.push_back((uint32_t)(2000 + j)); groups.push_back(2 + 2 * j); }
        for (size_t j = 0; j < 130; ++j) { items.push_back((uint32_t)(3000 + 7 * j)); groups.push_back(12); }
        check_subset(items, groups, 14, "a segment boundary at 63 / 64 / 65");
        std::vector<size_t> order(items.size());                            // the same choice, interleaved
        for (size_t j = 0; j < order.size(); ++j) order[j] = j;
        for (size_t j = order.size(); j > 1; --j) std::swap(order[j - 1], order[next64() % j]);
        std::vector<uint32_t> it2;
        std::vector<uint64_t> gr2;
        for (size_t j : order) { it2.push_back(items[j]); gr2.push_back(groups[j]); }
        check_subset(it2, gr2, 14, "the same, interleaved");
    }
    for (int round = 0; round < 50; ++round) {
        const size_t all = 1 + next64() % 700, n_groups = 1 + next64() % 40;
        std::vector<uint32_t> items;
        std::vector<uint64_t> groups;
        for (size_t i = 0; i < all; ++i) if (next64() % 3 == 0) { items.push_back((uint32_t)i); groups.push_back(next64() % n_groups); }
        check_subset(items, groups, n_groups, "a random subset");
    }
    {                                                                       // the second level of the entry: every chosen item its own group
        std::vector<uint32_t> items;
        std::vector<uint64_t> own;
        for (size_t j = 0; j < 200; ++j) { items.push_back((uint32_t)(5 * j + 3)); own.push_back(j); }
        check_subset(items, own, items.size(), "single items");
        LocatePlan p;
        locate_subset_plan(items.data(), own.data(), items.size(), items.size(), &p);
        EXPECT(p.segs.size() == 200 && p.part_off.back() == 200, "single items: one segment and one slot each");
        for (size_t j = 0; j < 200; ++j) EXPECT(p.segs[j] == j && p.perm[j] == items[j], "single items: segment %zu is chosen item %zu", j, j);
    }
    const uint64_t bad_group[2] = {0, 4};
    const uint32_t two[2] = {1, 2};
    LocatePlan p;
    EXPECT(locate_check_groups(bad_group, 2, 4) == KZG_ERR_INVALID_ARG && locate_check_groups(bad_group, 2, 5) == KZG_OK, "a group index = n_groups");
    EXPECT(locate_subset_plan(two, bad_group, 0, LOCATE_MAX_GROUPS + 1, &p) == KZG_ERR_TOO_LARGE, "n_groups > 2^28");
}

// ---- 2. the choice ---------------------------------------------------------------------------------------------------------------------------
static void check_choice() {
    const size_t B = 6, count = 7, use = 4;
    const uint8_t G = RETRIEVE_ITEM_GOOD;
    const uint8_t status[B * count] = {
        G, G, G, G, G, G, G,             // 0: nothing bad: the first four
        1, 2, 3, G, G, G, G,             // 1: bad items first, exactly use_count good ones
        G, G, G, G, 4, 1, 3,             // 2: bad items last
        G, 1, G, 4, G, 2, 3,             // 3: use_count - 1 good ones
        1, 2, 3, 4, 1, 2, 3,             // 4: every item bad
        G, 2, G, 1, G, 4, G,             // 5: interleaved
    };
    std::vector<uint32_t> chosen;
    std::vector<uint8_t> blob_status;
    const size_t un = retrieve_choose(status, B, count, use, &chosen, &blob_status);
    const uint32_t want[B][use] = {{0, 1, 2, 3}, {3, 4, 5, 6}, {0, 1, 2, 3}, {0, 1, 2, 3}, {0, 1, 2, 3}, {0, 2, 4, 6}};
    const uint8_t want_status[B] = {0, 0, 0, 1, 1, 0};
    EXPECT(un == 2 && chosen.size() == B * use && blob_status.size() == B, "choice: sizes and the number of blobs not recovered");
    for (size_t b = 0; b < B; ++b) {
        EXPECT(blob_status[b] == want_status[b], "choice: status of blob %zu", b);
        EXPECT(memcmp(chosen.data() + b * use, want[b], sizeof want[b]) == 0, "choice: positions of blob %zu", b);
    }
    EXPECT(retrieve_choose(status, B, count, count, &chosen, &blob_status) == 5 && blob_status[0] == 0, "use_count = count: only the clean blob");
    EXPECT(retrieve_choose(status, B, count, 1, &chosen, &blob_status) == 1 && blob_status[4] == 1 && chosen[1] == 3 && chosen[3] == 0, "use_count = 1");
}

// ---- 3. the planner of the recovery from chosen items ------------------------------------------------------------------------------------------
static void check_selected(const uint64_t* ks, size_t index_rows, size_t B, size_t count, size_t use, const uint8_t* status, size_t n, size_t l, size_t budget,
                           const char* what) {
    const size_t m = n / l;
    std::vector<uint32_t> chosen;
    std::vector<uint8_t> blob_status;
    retrieve_choose(status, B, count, use, &chosen, &blob_status);
    RecoverBatchPlan p, q;
    recover_selected_plan(ks, index_rows, B, count, use, chosen.data(), blob_status.data(), n, l, 0, true, 0, budget, &p);
    std::vector<uint64_t> rows(B * use);                                    // the chosen cosets as the rows of the existing planner
    for (size_t b = 0; b < B; ++b)
        for (size_t j = 0; j < use; ++j) rows[b * use + j] = ks[(index_rows == 1 ? 0 : b) * count + chosen[b * use + j]];
    const size_t want_rows = p.index_rows;
    EXPECT(want_rows == 1 || want_rows == B, "%s: index rows", what);
    recover_batch_plan(rows.data(), want_rows, B, use, n, l, 0, true, 0, budget, &q);
    EXPECT(p.held == count && p.value_stride() == count && q.value_stride() == use, "%s: the held stride", what);
    EXPECT(p.count == use && p.n_missing == m - use && p.degree_bound == use * l && p.out_len == n && p.blobs == B, "%s: the shape", what);
    EXPECT(p.missing == q.missing && p.pattern_of == q.pattern_of && p.n_patterns == q.n_patterns, "%s: patterns and missing lists", what);
    EXPECT(p.groups.group == q.groups.group && p.groups.n_groups == q.groups.n_groups && p.groups.blob_bytes == q.groups.blob_bytes, "%s: the grouping", what);
    EXPECT(p.w_item == q.w_item && p.w_pat == q.w_pat && p.w_miss == q.w_miss && p.w_flag == q.w_flag && p.w_zdom == q.w_zdom && p.w_zsinv == q.w_zsinv &&
           p.w_part == q.w_part && p.w_end == q.w_end, "%s: the layout (flags included)", what);
    EXPECT(p.item_of.size() == want_rows * m, "%s: the item map's size", what);
    for (size_t r = 0; r < want_rows; ++r)
        for (size_t k = 0; k < m; ++k) {
            const uint32_t at = p.item_of[r * m + k], in_rows = q.item_of[r * m + k];
            if (blob_status[r]) { EXPECT(at == RECOVER_NO_ITEM, "%s: a blob that is not recovered reads an item", what); continue; }
            EXPECT((at == RECOVER_NO_ITEM) == (in_rows == RECOVER_NO_ITEM), "%s: row %zu coset %zu present / missing", what, r, k);
            if (at == RECOVER_NO_ITEM || in_rows == RECOVER_NO_ITEM) continue;
            EXPECT(at < count && at == chosen[r * use + in_rows], "%s: row %zu coset %zu does not point into the held layout", what, r, k);
            EXPECT(ks[(index_rows == 1 ? 0 : r) * count + at] == k && status[r * count + at] == RETRIEVE_ITEM_GOOD, "%s: row %zu coset %zu names another chunk", what, r, k);
        }
    if (want_rows == 1 && index_rows == 1) for (size_t b = 0; b < B; ++b) EXPECT(!blob_status[b], "%s: one row although a blob is not recovered", what);
}

static void check_selected_plans() {
    const size_t n = 64, l = 4, B = 4, count = 7;
    const uint64_t ks[B * count] = {3, 0, 9, 14, 5, 1, 8, 1, 2, 3, 4, 5, 6, 7, 15, 0, 7, 8, 2, 9, 11, 3, 0, 9, 14, 5, 1, 8};
    const uint8_t G = 0;
    const uint8_t clean[B * count] = {};
    const uint8_t mixed[B * count] = {G, 1, G, G, 2, G, G, 3, 4, 1, G, G, G, G, G, G, G, G, 1, 1, 1, 1, 1, G, 4, G, 2, 3};
    check_selected(ks, B, B, count, count, clean, n, l, 0, "nothing bad, every item used");
    check_selected(ks, B, B, count, 4, clean, n, l, 0, "nothing bad, four of seven");
    check_selected(ks, B, B, count, 4, mixed, n, l, 0, "mixed (the last blob is not recovered)");
    check_selected(ks, B, B, count, 3, mixed, n, l, 1, "mixed, groups of one blob");
    check_selected(ks, 1, B, count, count, clean, n, l, 0, "one index row, nothing bad: one row");
    check_selected(ks, 1, B, count, 4, clean, n, l, 0, "one index row, four of seven: one row");
    check_selected(ks, 1, B, count, 4, mixed, n, l, 0, "one index row, mixed: a row per blob");
    {
        std::vector<uint32_t> chosen;
        std::vector<uint8_t> bs;
        RecoverBatchPlan p;
        retrieve_choose(clean, B, count, 4, &chosen, &bs);
        recover_selected_plan(ks, 1, B, count, 4, chosen.data(), bs.data(), n, l, 0, true, 0, 0, &p);
        EXPECT(p.index_rows == 1 && p.n_patterns == 1, "equal choices under one index row are one row and one pattern");
        retrieve_choose(mixed, B, count, 4, &chosen, &bs);
        recover_selected_plan(ks, 1, B, count, 4, chosen.data(), bs.data(), n, l, 0, true, 0, 0, &p);
        EXPECT(p.index_rows == B, "different choices under one index row are a row per blob");
    }
}

// ---- 4. the table of kzg_retrieve_blobs_bytes_tolerant, in its order -------------------------------------------------------------------------
static void check_table() {
    const size_t n = 64, l = 4, m = n / l, B = 3, count = 5, use = 3;
    const uint64_t ks[B * count] = {3, 0, 9, 14, 5, 1, 2, 3, 4, 5, 15, 0, 7, 8, 2};
    auto call = [&](bool any_null, const uint64_t* idx, size_t rows, size_t blobs, size_t cnt, size_t use_, size_t n_, size_t l_, size_t bound, bool form, size_t out_len) {
        return retrieve_tolerant_check(any_null, idx, rows, blobs, cnt, use_, n_, l_, bound, form, out_len);
    };
    EXPECT(call(false, ks, B, B, count, use, n, l, 0, false, 0) == KZG_OK && call(false, ks, 1, B, count, count, n, l, 0, true, n) == KZG_OK &&
           call(false, ks, B, B, count, 1, n, l, 0, false, 0) == KZG_OK, "a valid call is refused");
    EXPECT(call(true, ks, 2, B, count, use, 0, l, 0, false, 0) == KZG_ERR_INVALID_ARG, "1. a null pointer in front of everything");
    EXPECT(call(false, ks, 1, 0, count, use, 0, l, 0, false, 0) == KZG_ERR_INVALID_ARG, "1. blobs = 0 in front of n = 0");
    EXPECT(call(false, ks, 2, B, count, use, 0, l, 0, false, 0) == KZG_ERR_INVALID_ARG, "2. index_rows neither 1 nor blobs, in front of n = 0");
    EXPECT(call(false, ks, B, B, count, 0, 0, l, 0, false, 0) == KZG_ERR_NOT_POWER_OF_TWO, "3. n = 0 in front of use_count = 0");
    EXPECT(call(false, ks, B, B, count, use, 96, 3, 0, false, 0) == KZG_ERR_NOT_POWER_OF_TWO, "3. n = 96 in front of l = 3");
    EXPECT(call(false, ks, B, B, count, use, (size_t)1 << 25, 3, 0, false, 0) == KZG_ERR_DOMAIN, "3. n = 2^25 in front of l = 3");
    EXPECT(call(false, ks, B, B, count, use, 1, 1, 0, false, 0) == KZG_ERR_INVALID_ARG, "3. n = 1");
    EXPECT(call(false, ks, B, B, count, use, n, 0, 0, false, 0) == KZG_ERR_INVALID_ARG && call(false, ks, B, B, count, use, n, 3, 0, false, 0) == KZG_ERR_INVALID_ARG &&
           call(false, ks, B, B, count, use, n, 64, 0, false, 0) == KZG_ERR_INVALID_ARG, "3. the chunk length");
    EXPECT(call(false, ks, B, B, 0, 0, n, l, 0, false, 0) == KZG_ERR_INVALID_ARG && call(false, ks, B, B, m + 1, use, n, l, 0, false, 0) == KZG_ERR_INVALID_ARG, "3. count");
    uint64_t bad[B * count];
    memcpy(bad, ks, sizeof ks);
    bad[2 * count + 4] = m;                                                 // (a held item beyond the first use_count: every held index is checked)
    EXPECT(call(false, bad, B, B, count, 0, n, l, 0, false, 0) == KZG_ERR_INVALID_ARG && call(false, bad, B, B, count, count + 1, n, l, 0, false, 0) == KZG_ERR_INVALID_ARG,
           "3. use_count = 0 and use_count > count, in front of the indices");
    EXPECT(call(false, bad, B, B, count, use, n, l, 99, false, 0) == KZG_ERR_INVALID_ARG, "4. an index = m in the last row, in front of the bound");
    memcpy(bad, ks, sizeof ks);
    bad[count + 4] = 1;
    EXPECT(call(false, bad, B, B, count, use, n, l, 0, false, 0) == KZG_ERR_INVALID_ARG, "4. a duplicate in the middle row");
    EXPECT(call(false, bad, 1, B, count, use, n, l, 0, false, 0) == KZG_OK, "4. with one index row only the first row is read");
    EXPECT(call(false, ks, B, B, count, use, n, l, use * l, false, 0) == KZG_OK && call(false, ks, B, B, count, use, n, l, use * l + 1, false, 1) == KZG_ERR_INVALID_ARG &&
           call(false, ks, B, B, count, count, n, l, use * l + 1, false, 0) == KZG_OK, "5. the degree bound against use_count x l, in front of out_len");
    EXPECT(call(false, ks, B, B, count, use, n, l, 0, false, use * l - 1) == KZG_ERR_INVALID_ARG && call(false, ks, B, B, count, use, n, l, 0, false, use * l) == KZG_OK &&
           call(false, ks, B, B, count, use, n, l, 0, false, n + 1) == KZG_ERR_INVALID_ARG && call(false, ks, B, B, count, use, n, l, 0, true, n - 1) == KZG_ERR_INVALID_ARG,
           "6. out_len against use_count x l");
    {                                                                       // 7. the cost cap counts m - use_count missing cosets
        const size_t cn = (size_t)1 << 24, cm = cn;                         // l = 1: m = 2^24; m (m - use) <= 2^32 needs use >= m - 256
        std::vector<uint64_t> all(cm);
        for (size_t i = 0; i < cm; ++i) all[i] = i;
        EXPECT(call(false, all.data(), 1, 1, cm, cm - 256, cn, 1, 0, false, 0) == KZG_OK, "7. m - use_count = 256 missing cosets pass");
        EXPECT(call(false, all.data(), 1, 1, cm, cm - 257, cn, 1, 0, false, 0) == KZG_ERR_TOO_LARGE, "7. the cost cap of one blob, on use_count although every coset is held");
        EXPECT(call(false, all.data(), 1, 1, cm, cm - 257, cn, 1, 0, true, 2) == KZG_ERR_INVALID_ARG, "6 in front of 7");
    }
    EXPECT(call(false, ks, 1, SIZE_MAX / (n * 32) + 1, count, use, n, l, 0, false, 0) == KZG_ERR_INVALID_ARG, "8. the batch's arrays overflow size_t");
    {                                                                       // 9. the cap on the values of a call counts the HELD items
        const size_t cn = (size_t)1 << 20, cl = (size_t)1 << 10, cm = cn / cl;
        std::vector<uint64_t> all(cm);
        for (size_t i = 0; i < cm; ++i) all[i] = i;
        EXPECT(call(false, all.data(), 1, 256, cm, cm / 2, cn, cl, 0, false, 0) == KZG_OK, "9. 2^28 held values pass");
        EXPECT(call(false, all.data(), 1, 257, cm, cm / 2, cn, cl, 0, false, 0) == KZG_ERR_TOO_LARGE, "9. more than 2^28 held values");
        EXPECT(call(false, all.data(), 1, 257, cm, cm / 2, cn, cl, 0, true, 5) == KZG_ERR_INVALID_ARG, "6 in front of 9");
    }
    // with use_count = count the table is that of kzg_retrieve_blobs_bytes's recovery half
    for (size_t bound : {(size_t)0, (size_t)8, count * l, count * l + 1})
        for (size_t out_len : {(size_t)0, (size_t)7, (size_t)8, n, n + 1})
            for (int form = 0; form < 2; ++form)
                EXPECT(call(false, ks, B, B, count, count, n, l, bound, form != 0, out_len) == recover_bytes_check(false, ks, B, B, count, n, l, bound, form != 0, out_len),
                       "use_count = count: bound %zu out_len %zu form %d differs from recover_bytes_check", bound, out_len, form);
}

int main() {
    check_subset_plans();
    check_choice();
    check_selected_plans();
    check_table();
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    printf("retrievetolerantcheck ok\n");
    return 0;
}
