// recoverbatchcheck.cpp -- the batch plan of csrc/host_recover.h as a plain host program (g++ -fsanitize=address,undefined, no GPU, no
// library): every error of kzg_recover_from_cosets_batch's table in its order, the deduplication of missing sets into patterns,
// pattern_of and item_of, the group sizes over a grid of (shape, budget, blobs), the word layout against the highest word a group
// addresses, what one upload carries, the split of the vanishing products, and the single call as the batch of one.
// Prints "recoverbatchcheck ok"; a failed check prints its line and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_recover.h"

using namespace kzg;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "recoverbatchcheck: line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)

typedef std::vector<uint64_t> Idx;
typedef std::vector<uint32_t> U32;

static int32_t check_of(const Idx& ks, size_t index_rows, size_t blobs, size_t count, size_t n, size_t l, size_t bound, bool eval_form, size_t out_len,
                        bool any_null = false) {
    return recover_batch_check(any_null, ks.data(), index_rows, blobs, count, n, l, bound, eval_form, out_len);
}
static RecoverBatchPlan plan_of(const Idx& ks, size_t index_rows, size_t blobs, size_t count, size_t n, size_t l, size_t bound = 0, bool eval_form = true,
                                size_t out_len = 0, size_t budget = 0) {
    CHECK(check_of(ks, index_rows, blobs, count, n, l, bound, eval_form, out_len) == KZG_OK);
    RecoverBatchPlan p;
    recover_batch_plan(ks.data(), index_rows, blobs, count, n, l, bound, eval_form, out_len, budget, &p);
    return p;
}
static U32 slice(const U32& v, size_t from, size_t len) { return U32(v.begin() + from, v.begin() + from + len); }

int main() {
    // ---- the error table, each case wrong in its own row AND in later rows that can be wrong at the same time: the earlier wins
    const Idx two = {0, 1}, dup = {1, 1}, high = {0, 4};
    CHECK(check_of(dup, 3, 2, 2, 0, 3, 99, true, 5, true) == KZG_ERR_INVALID_ARG);                 // 1. a null pointer, in front of everything
    CHECK(check_of(dup, 3, 0, 2, 0, 3, 99, true, 5) == KZG_ERR_INVALID_ARG);                       //    blobs = 0, in front of a bad index_rows and n
    CHECK(check_of(dup, 3, 2, 2, 0, 3, 99, true, 5) == KZG_ERR_INVALID_ARG);                       // 2. index_rows = 3 of 2 blobs, in front of n = 0
    CHECK(check_of(dup, 0, 2, 2, 16, 4, 0, true, 0) == KZG_ERR_INVALID_ARG);                       //    index_rows = 0
    CHECK(check_of(dup, 1, 2, 2, 0, 3, 99, true, 5) == KZG_ERR_NOT_POWER_OF_TWO);                  // 3. n = 0
    CHECK(check_of(dup, 1, 2, 2, 24, 3, 99, true, 5) == KZG_ERR_NOT_POWER_OF_TWO);                 //    n not a power of two
    CHECK(check_of(dup, 1, 2, 2, (size_t)1 << 25, 3, 99, true, 5) == KZG_ERR_DOMAIN);              //    n > 2^24, in front of a bad chunk length
    CHECK(check_of(dup, 1, 2, 2, 1, 1, 99, true, 5) == KZG_ERR_INVALID_ARG);                       //    n = 1
    CHECK(check_of(two, 1, 2, 2, 16, 0, 0, true, 0) == KZG_ERR_INVALID_ARG);                       //    l = 0
    CHECK(check_of(two, 1, 2, 2, 16, 3, 0, true, 0) == KZG_ERR_INVALID_ARG);                       //    l not a power of two
    CHECK(check_of(two, 1, 2, 2, 16, 16, 0, true, 0) == KZG_ERR_INVALID_ARG);                      //    l > n / 2
    CHECK(check_of(two, 1, 2, 0, 16, 4, 0, true, 0) == KZG_ERR_INVALID_ARG);                       //    count = 0
    CHECK(check_of({0, 1, 2, 3, 0}, 1, 2, 5, 16, 4, 0, true, 0) == KZG_ERR_INVALID_ARG);           //    count > m
    CHECK(check_of(high, 1, 2, 2, 16, 4, 99, true, 5) == KZG_ERR_INVALID_ARG);                     // 4. an index = m, in front of the bound and out_len
    CHECK(check_of({0, ~(uint64_t)0}, 1, 2, 2, 16, 4, 0, true, 0) == KZG_ERR_INVALID_ARG);         //    an index far outside
    CHECK(check_of(dup, 1, 2, 2, 16, 4, 0, true, 0) == KZG_ERR_INVALID_ARG);                       //    a duplicate
    CHECK(check_of({0, 1, 2, 2}, 2, 2, 2, 16, 4, 0, true, 0) == KZG_ERR_INVALID_ARG);              //    a duplicate in the second row only
    CHECK(check_of({0, 1, 1, 0}, 2, 2, 2, 16, 4, 0, true, 0) == KZG_OK);                           //    the same coset in two rows is no duplicate
    CHECK(check_of(two, 1, 2, 2, 16, 4, 9, true, 5) == KZG_ERR_INVALID_ARG);                       // 5. degree_bound = count l + 1, in front of out_len
    CHECK(check_of({0}, 1, 2, 1, (size_t)1 << 24, 1, 2, true, 0) == KZG_ERR_INVALID_ARG);          //    ... and of the cap
    CHECK(check_of(two, 1, 2, 2, 16, 4, 0, true, 8) == KZG_ERR_INVALID_ARG);                       // 6. evaluations with out_len != n
    CHECK(check_of(two, 1, 2, 2, 16, 4, 0, true, 16) == KZG_OK && check_of(two, 1, 2, 2, 16, 4, 0, true, 0) == KZG_OK);
    CHECK(check_of(two, 1, 2, 2, 16, 4, 0, false, 7) == KZG_ERR_INVALID_ARG);                      //    coefficients: below the resolved bound 8
    CHECK(check_of(two, 1, 2, 2, 16, 4, 5, false, 4) == KZG_ERR_INVALID_ARG);                      //    ... below the given bound 5
    CHECK(check_of(two, 1, 2, 2, 16, 4, 5, false, 17) == KZG_ERR_INVALID_ARG);                     //    ... above n
    CHECK(check_of(two, 1, 2, 2, 16, 4, 5, false, 5) == KZG_OK && check_of(two, 1, 2, 2, 16, 4, 0, false, 8) == KZG_OK);
    CHECK(check_of({0}, 1, 2, 1, (size_t)1 << 24, 1, 1, true, 3) == KZG_ERR_INVALID_ARG);          //    ... in front of the cap
    CHECK(check_of({0}, 1, SIZE_MAX, 1, (size_t)1 << 24, 1, 1, true, 0) == KZG_ERR_TOO_LARGE);     // 7. the cap, in front of the overflow
    CHECK(check_of(two, 1, SIZE_MAX / 512 + 1, 2, 16, 4, 0, true, 0) == KZG_ERR_INVALID_ARG);      // 8. blobs x 16 x 32 bytes overflow
    CHECK(check_of(two, 1, SIZE_MAX / 512, 2, 16, 4, 0, true, 0) == KZG_OK);
    // the query's checks: the shape rows, out_len <= n, rows 7 and 8
    CHECK(recover_batch_info_check(true, 0, 2, 0, 3, 99) == KZG_ERR_INVALID_ARG);
    CHECK(recover_batch_info_check(false, 0, 2, 0, 3, 99) == KZG_ERR_INVALID_ARG);
    CHECK(recover_batch_info_check(false, 2, 2, 0, 3, 99) == KZG_ERR_NOT_POWER_OF_TWO);
    CHECK(recover_batch_info_check(false, 2, 2, (size_t)1 << 25, 3, 0) == KZG_ERR_DOMAIN);
    CHECK(recover_batch_info_check(false, 2, 5, 16, 4, 0) == KZG_ERR_INVALID_ARG);
    CHECK(recover_batch_info_check(false, 2, 2, 16, 4, 17) == KZG_ERR_INVALID_ARG);
    CHECK(recover_batch_info_check(false, 2, 1, (size_t)1 << 24, 1, 0) == KZG_ERR_TOO_LARGE);
    CHECK(recover_batch_info_check(false, SIZE_MAX / 512 + 1, 2, 16, 4, 0) == KZG_ERR_INVALID_ARG);
    CHECK(recover_batch_info_check(false, 7, 2, 16, 4, 16) == KZG_OK);

    // ---- patterns: m = 8, count = 5.  Rows 0, 3, 5 hold the set {0, 2, 3, 5, 7} in three orders, rows 1, 2 the set {1, 2, 3, 4, 5},
    // row 4 {0, 1, 2, 3, 4}, row 6 {7, 6, 5, 4, 3}
    {
        const Idx ks = {0, 2, 3, 5, 7,  1, 2, 3, 4, 5,  5, 4, 3, 2, 1,  7, 5, 3, 2, 0,  0, 1, 2, 3, 4,  3, 0, 7, 2, 5,  7, 6, 5, 4, 3};
        const RecoverBatchPlan p = plan_of(ks, 7, 7, 5, 32, 4);
        CHECK(p.m == 8 && p.l == 4 && p.count == 5 && p.blobs == 7 && p.index_rows == 7 && p.n_missing == 3 && p.log_n == 5 && p.log_l == 2 && p.log_m == 3);
        CHECK(p.degree_bound == 20 && p.out_len == 32 && p.eval_form);
        CHECK(p.n_patterns == 4 && (p.pattern_of == U32{0, 1, 1, 0, 2, 0, 3}));                    // numbered in order of first appearance
        CHECK((p.missing == U32{1, 4, 6,  0, 6, 7,  5, 6, 7,  0, 1, 2}));                           // each ascending
        const uint32_t X = RECOVER_NO_ITEM;
        CHECK(p.item_of.size() == 7 * 8);
        CHECK((slice(p.item_of, 0, 8) == U32{0, X, 1, 2, X, 3, X, 4}));
        CHECK((slice(p.item_of, 3 * 8, 8) == U32{4, X, 3, 2, X, 1, X, 0}));                        // the same set, another order: another item map
        CHECK((slice(p.item_of, 5 * 8, 8) == U32{1, X, 3, 0, X, 4, X, 2}));
        CHECK((slice(p.item_of, 2 * 8, 8) == U32{X, 4, 3, 2, 1, 0, X, X}));
        for (size_t b = 0; b < 7; ++b) CHECK(p.blob_pattern(b) == p.pattern_of[b]);
        CHECK(p.groups.group == 7 && p.groups.n_groups == 1);
        // the upload of the whole call, and of groups of 3, 3, 1: patterns renumbered inside each group
        std::vector<uint32_t> st;
        size_t words = 0;
        CHECK(recover_batch_stage(p, 0, 7, &st, &words) == 4 && words == p.w_miss + 4 * 3 && st.size() == p.w_flag);
        CHECK(slice(st, p.w_item, 56) == p.item_of && (slice(st, p.w_pat, 7) == U32{0, 1, 1, 0, 2, 0, 3}) && slice(st, p.w_miss, 12) == p.missing);
        RecoverBatchPlan q = plan_of(ks, 7, 7, 5, 32, 4, 0, true, 0, 3 * p.groups.blob_bytes);
        CHECK(q.groups.group == 3 && q.groups.n_groups == 3 && q.groups.blob_bytes == p.groups.blob_bytes && q.groups.group_bytes == 3 * q.groups.blob_bytes + 16);
        CHECK(recover_batch_stage(q, 0, 3, &st, &words) == 2 && words == q.w_miss + 6);
        CHECK((slice(st, q.w_pat, 3) == U32{0, 1, 1}) && (slice(st, q.w_miss, 6) == U32{1, 4, 6, 0, 6, 7}) && slice(st, 0, 24) == slice(p.item_of, 0, 24));
        CHECK(recover_batch_stage(q, 3, 3, &st, &words) == 2 && words == q.w_miss + 6);
        CHECK((slice(st, q.w_pat, 3) == U32{0, 1, 0}) && (slice(st, q.w_miss, 6) == U32{1, 4, 6, 5, 6, 7}) && slice(st, 0, 24) == slice(p.item_of, 24, 24));
        CHECK(recover_batch_stage(q, 6, 1, &st, &words) == 1 && words == q.w_miss + 3);
        CHECK(st[q.w_pat] == 0 && (slice(st, q.w_miss, 3) == U32{0, 1, 2}) && slice(st, 0, 8) == slice(p.item_of, 48, 8));
    }
    {   // one index row: one pattern, one item map, whatever the number of blobs; the upload does not grow with the blobs
        const RecoverBatchPlan p = plan_of({3, 0}, 1, 1000, 2, 16, 4, 5, false, 6);
        CHECK(p.n_patterns == 1 && (p.pattern_of == U32{0}) && (p.missing == U32{1, 2}) && (p.item_of == U32{1, RECOVER_NO_ITEM, RECOVER_NO_ITEM, 0}));
        CHECK(p.degree_bound == 5 && p.out_len == 6 && !p.eval_form && p.blob_pattern(999) == 0);
        std::vector<uint32_t> st;
        size_t words = 0;
        CHECK(recover_batch_stage(p, 0, 1000, &st, &words) == 1 && words == p.w_miss + 2 && p.w_pat == 4 && p.w_miss == 4 + 1000);
        for (size_t b = 0; b < 1000; ++b) CHECK(st[p.w_pat + b] == 0);
        // the single call is this plan with one blob
        RecoverPlan one;
        CHECK(recover_plan(false, Idx{3, 0}.data(), 2, 16, 4, 5, &one) == KZG_OK);
        const RecoverBatchPlan s = recover_batch_of_one(one, false);
        const RecoverBatchPlan t = plan_of({3, 0}, 1, 1, 2, 16, 4, 5, false, 0);
        CHECK(s.missing == t.missing && s.item_of == t.item_of && s.pattern_of == t.pattern_of && s.n_patterns == 1 && s.out_len == 16 && s.degree_bound == 5);
        CHECK(s.w_item == t.w_item && s.w_pat == t.w_pat && s.w_miss == t.w_miss && s.w_flag == t.w_flag && s.w_zdom == t.w_zdom && s.w_zsinv == t.w_zsinv &&
              s.w_part == t.w_part && s.w_end == t.w_end && s.groups.group == 1 && s.groups.n_groups == 1);
    }
    {   // nothing missing: an empty pattern, shared by every order of the items
        const RecoverBatchPlan p = plan_of({0, 1, 2, 3,  3, 2, 1, 0}, 2, 2, 4, 16, 4);
        CHECK(p.n_patterns == 1 && p.n_missing == 0 && p.missing.empty() && (p.pattern_of == U32{0, 0}));
        CHECK((p.item_of == U32{0, 1, 2, 3, 3, 2, 1, 0}));
    }

    // ---- groups over a grid of (shape, budget, blobs): never 0, never above the blobs or grid.y, inside the budget unless one blob alone
    // exceeds it, the ragged last group, monotone in the budget; the layout covers every word a full group addresses
    const size_t shapes[][3] = {{8, 4, 1}, {64, 4, 9}, {2048, 16, 64}, {4096, 1, 2048}, {4096, 16, 256}, {(size_t)1 << 13, 1, 4096}, {(size_t)1 << 16, 64, 512},
                                {(size_t)1 << 20, 16, 65535}, {(size_t)1 << 24, 2, ((size_t)1 << 23) - 512}};
    const size_t blob_counts[] = {1, 2, 7, 64, 32768, 100000};
    for (const auto& sh : shapes) {
        const size_t n = sh[0], l = sh[1], count = sh[2], m = n / l;
        for (size_t blobs : blob_counts) {
            size_t prev = 0;
            for (size_t budget : {(size_t)1, (size_t)4096, (size_t)1 << 20, (size_t)1 << 26, (size_t)1 << 32, (size_t)1 << 40}) {
                const RecoverBatchGroups g = recover_batch_groups(blobs, count, n, l, budget);
                CHECK(g.group >= 1 && g.group <= blobs && g.group <= RECOVER_GROUP_MAX && g.budget == budget);
                CHECK(g.group_bytes == g.group * g.blob_bytes + 16 && (g.group == 1 || g.group * g.blob_bytes <= budget));
                CHECK(g.group == blobs || g.group == RECOVER_GROUP_MAX || (g.group + 1) * g.blob_bytes > budget);     // the largest group that fits
                CHECK(g.n_groups == (blobs + g.group - 1) / g.group && (g.n_groups - 1) * g.group < blobs);
                CHECK(g.group >= prev);
                prev = g.group;
            }
            const RecoverBatchGroups d = recover_batch_groups(blobs, count, n, l, 0), e = recover_batch_groups(blobs, count, n, l, (size_t)4 << 30);
            CHECK(d.budget == RECOVER_GROUP_BYTES_DEFAULT && d.group == e.group && d.group_bytes == e.group_bytes);
        }
        // the bytes of a blob cover its share of every array: values, staging, item map, pattern, missing list, flag, vanishing values, partials
        const RecoverBatchGroups g1 = recover_batch_groups(1, count, n, l, 0);
        const RecoverSplit sp1 = recover_vanish_split(m, m - count, 1);
        CHECK(g1.blob_bytes >= 64 * n + 4 * (m + 2 + (m - count)) + 72 * m + (size_t)sp1.splits * 72 * m);
        // the split: every root in exactly one slice, all patterns together near the target, never more splits than with one pattern
        for (size_t P : {(size_t)1, (size_t)2, (size_t)7, (size_t)64, (size_t)32768}) {
            const RecoverSplit sp = recover_vanish_split(m, m - count, P);
            CHECK(sp.xgroups == (2 * m + 255) / 256 && sp.tiles == (m - count + 255) / 256);
            CHECK(sp.splits >= 1 && sp.splits <= sp1.splits && sp.per_split % RECOVER_TILE == 0 && sp.per_split >= RECOVER_TILE);
            CHECK((uint64_t)sp.splits * sp.per_split >= m - count);
            CHECK(sp.splits == 1 || (uint64_t)(sp.splits - 1) * sp.per_split < m - count);        // no empty slice but the only one
            CHECK(sp.splits == 1 || (uint64_t)sp.splits * sp.xgroups * P <= RECOVER_TARGET_GROUPS);
        }
    }
    {   // the layout of a plan with `group` index rows: the regions in order, the planes 16-byte aligned, the end covering P = group patterns
        std::vector<uint64_t> ks;
        for (size_t b = 0; b < 5; ++b)
            for (uint64_t i = 0; i < 100; ++i) ks.push_back((i * 3 + b) % 256);                    // five different sets of 100 of m = 256 cosets
        const RecoverBatchPlan p = plan_of(ks, 5, 5, 100, 4096, 16);
        CHECK(p.n_patterns == 5 && p.groups.group == 5);
        const RecoverSplit sp1 = recover_vanish_split(256, 156, 1);
        CHECK(p.w_item == 0 && p.w_pat == 5 * 256 && p.w_miss == p.w_pat + 5 && p.w_flag == p.w_miss + 5 * 156 && p.w_zdom >= p.w_flag + 5 && p.w_zdom % 4 == 0);
        CHECK(p.w_zsinv == p.w_zdom + 5 * 9 * 256 && p.w_part == p.w_zsinv + 5 * 9 * 256 && p.w_end == p.w_part + 5 * sp1.splits * 9 * 512);
        CHECK(p.w_end * 4 <= p.groups.group_bytes - 2 * 5 * 4096 * 32);                            // the small arrays fit what the grouping counted for them
        for (size_t P = 1; P <= 5; ++P) {                                                         // pattern z's partials end inside the region
            const RecoverSplit sp = recover_vanish_split(256, 156, P);
            CHECK(p.w_part + P * sp.splits * 9 * 512 <= p.w_end);
        }
    }
    printf("recoverbatchcheck ok\n");
    return 0;
}
