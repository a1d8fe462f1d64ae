// host_recover.h — the host side of kzg_recover_from_cosets (recover.hip, capi_verify.hip): every argument check of the entry, in the
// order the header documents, and what the kernels need from the coset indices -- the sorted list of the MISSING cosets (the roots of
// the vanishing polynomial) and, per coset, the item that carries its values.  Nothing here grows with n: the work is O(m), m = n / l.
// kzg_recover_from_cosets_batch adds the plan of a batch (below): the checks of its table, the blobs' missing sets deduplicated into
// PATTERNS, the grouping by a byte budget, the word layout of a group's small arrays and the host array one upload carries.
// The serialized-form entries (kzg_recover_from_cosets_batch_bytes, kzg_retrieve_blobs_bytes) add their table and the blobs' chunks as verifier items.
// Pure host code: no HIP type, no kzg_ctx, no device call; also compiled with g++ by tests/hostcheck/recovercheck.cpp,
// tests/hostcheck/recoverbatchcheck.cpp and tests/hostcheck/recoverbytescheck.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

#include "../../include/kzg_bn254_mi355x.h"
#include "ntt_plan.h"

namespace kzg {

constexpr size_t RECOVER_MAX_N = (size_t)1 << 24;
// The vanishing values are direct products: 2 m |M| field products for |M| missing cosets.  m |M| <= 2^32 admits every (n, l) with
// m <= 2^16 whatever is missing (2^33 products, a few tens of milliseconds) and larger m with proportionally fewer missing cosets.
constexpr uint64_t RECOVER_MAX_PRODUCTS = (uint64_t)1 << 32;
constexpr uint32_t RECOVER_NO_ITEM = 0xFFFFFFFFu;

struct RecoverPlan {
    size_t n = 0, l = 0, m = 0, count = 0;
    int log_n = 0, log_l = 0, log_m = 0;
    size_t degree_bound = 0;               // resolved: 0 of the caller -> count l
    std::vector<uint32_t> missing;         // the cosets without an item, ascending: m - count entries
    std::vector<uint32_t> item_of;         // [coset] -> its item, RECOVER_NO_ITEM for a missing coset: m entries
};

// The checks 2 .. 8 of the header's table (1, the null pointers, is `any_null`), then the plan.  On an error the plan is left empty.
inline int32_t recover_plan(bool any_null, const uint64_t* coset_indices, size_t count, size_t n, size_t chunk_len, size_t degree_bound,
                            RecoverPlan* plan) {
    *plan = RecoverPlan();
    if (any_null) return KZG_ERR_INVALID_ARG;
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_NOT_POWER_OF_TWO;
    if (n > RECOVER_MAX_N) return KZG_ERR_DOMAIN;
    const size_t l = chunk_len;
    if (n == 1 || l == 0 || (l & (l - 1)) != 0 || l > n / 2) return KZG_ERR_INVALID_ARG;
    const size_t m = n / l;
    if (count == 0 || count > m) return KZG_ERR_INVALID_ARG;
    std::vector<uint64_t> seen((m + 63) / 64, 0);                    // one bit per coset: 256 KiB at m = 2^24
    for (size_t i = 0; i < count; ++i) {
        const uint64_t k = coset_indices[i];
        if (k >= m) return KZG_ERR_INVALID_ARG;
        uint64_t& word = seen[k >> 6];
        const uint64_t bit = (uint64_t)1 << (k & 63);
        if (word & bit) return KZG_ERR_INVALID_ARG;                  // the same coset twice
        word |= bit;
    }
    if (degree_bound > count * l) return KZG_ERR_INVALID_ARG;        // too few cosets for that degree
    if ((uint64_t)m * (uint64_t)(m - count) > RECOVER_MAX_PRODUCTS) return KZG_ERR_TOO_LARGE;
    plan->n = n; plan->l = l; plan->m = m; plan->count = count;
    plan->log_n = __builtin_ctzll(n); plan->log_l = __builtin_ctzll(l); plan->log_m = plan->log_n - plan->log_l;
    plan->degree_bound = degree_bound ? degree_bound : count * l;
    plan->item_of.assign(m, RECOVER_NO_ITEM);
    for (size_t i = 0; i < count; ++i) plan->item_of[coset_indices[i]] = (uint32_t)i;
    plan->missing.reserve(m - count);
    for (size_t k = 0; k < m; ++k)
        if (plan->item_of[k] == RECOVER_NO_ITEM) plan->missing.push_back((uint32_t)k);
    return KZG_OK;
}

// ---- kzg_recover_from_cosets_batch: `blobs` blobs of one shape (n, l, count, degree_bound, form) --------------------------------------
// The geometry of the vanishing-value kernels (recover.hip), here because the workspace of a group depends on it
constexpr uint32_t RECOVER_THREADS = 256;             // lanes of a workgroup: one output point each
constexpr uint32_t RECOVER_TILE = 256;                // roots per LDS tile
constexpr uint32_t RECOVER_TARGET_GROUPS = 1024;      // workgroups of k_recover_vanish in all: four waves per SIMD on 256 CUs
constexpr size_t RECOVER_LIMBS = 9;                   // words of a field element in limb planes (NL of field29.h)
// The default budget of a group's workspace: the encoder's (ENCODE_GROUP_BYTES_DEFAULT), one default for both batched calls -- a choice
// for consistency, not a measured optimum.  One blob needs ~10 MiB at (2^13, 1) with half missing (9 MiB of it
// partial products: 16 splits), ~4.2 MiB at (2^16, 64), ~78 MiB at (2^20, 16): 4 GiB holds 52 of the largest.
constexpr size_t RECOVER_GROUP_BYTES_DEFAULT = (size_t)4 << 30;
constexpr size_t RECOVER_GROUP_MAX = 32768;           // blobs per group: grid.y (and, for the patterns, grid.z) of a launch

// How the |M| roots of one pattern are split across workgroups when `patterns` patterns share the launch: all patterns together aim at
// RECOVER_TARGET_GROUPS workgroups.  patterns = 1 is the single call.  The fold gives the same element whatever the split.
struct RecoverSplit { uint32_t xgroups, tiles, splits, per_split; };
inline RecoverSplit recover_vanish_split(size_t m, size_t n_missing, size_t patterns) {
    RecoverSplit s;
    s.xgroups = (uint32_t)((2 * m + RECOVER_THREADS - 1) / RECOVER_THREADS);
    s.tiles = (uint32_t)((n_missing + RECOVER_TILE - 1) / RECOVER_TILE);
    const uint64_t across = (uint64_t)s.xgroups * std::max<size_t>(patterns, 1);
    s.splits = std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)(RECOVER_TARGET_GROUPS / across), s.tiles));
    s.per_split = std::max<uint32_t>(1, (s.tiles + s.splits - 1) / s.splits) * RECOVER_TILE;
    return s;
}

// rows 2 .. 5 of the single entry's table: the shape
inline int32_t recover_shape_check(size_t count, size_t n, size_t chunk_len) {
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_NOT_POWER_OF_TWO;
    if (n > RECOVER_MAX_N) return KZG_ERR_DOMAIN;
    const size_t l = chunk_len;
    if (n == 1 || l == 0 || (l & (l - 1)) != 0 || l > n / 2) return KZG_ERR_INVALID_ARG;
    if (count == 0 || count > n / l) return KZG_ERR_INVALID_ARG;
    return KZG_OK;
}
// rows 7 and 8 of the batch table: the cost cap of one blob, then a batch whose arrays overflow size_t (the largest is blobs x n x 32 bytes)
inline int32_t recover_batch_size_check(size_t blobs, size_t count, size_t n, size_t chunk_len) {
    const size_t m = n / chunk_len;
    if ((uint64_t)m * (uint64_t)(m - count) > RECOVER_MAX_PRODUCTS) return KZG_ERR_TOO_LARGE;
    if (blobs > SIZE_MAX / (n * 32)) return KZG_ERR_INVALID_ARG;
    return KZG_OK;
}

// Every check of kzg_recover_from_cosets_batch's table, in its order (1, the null pointers, is `any_null`).  Reads the indices, builds nothing.
inline int32_t recover_batch_check(bool any_null, const uint64_t* coset_indices, size_t index_rows, size_t blobs, size_t count, size_t n,
                                   size_t chunk_len, size_t degree_bound, bool eval_form, size_t out_len) {
    if (any_null || blobs == 0) return KZG_ERR_INVALID_ARG;
    if (index_rows != 1 && index_rows != blobs) return KZG_ERR_INVALID_ARG;
    const int32_t rc = recover_shape_check(count, n, chunk_len);
    if (rc != KZG_OK) return rc;
    const size_t l = chunk_len, m = n / l;
    std::vector<uint64_t> seen((m + 63) / 64);                       // one bit per coset, cleared per row
    for (size_t r = 0; r < index_rows; ++r) {
        std::fill(seen.begin(), seen.end(), 0);
        for (size_t i = 0; i < count; ++i) {
            const uint64_t k = coset_indices[r * count + i];
            if (k >= m) return KZG_ERR_INVALID_ARG;
            uint64_t& word = seen[k >> 6];
            const uint64_t bit = (uint64_t)1 << (k & 63);
            if (word & bit) return KZG_ERR_INVALID_ARG;              // the same coset twice in one row
            word |= bit;
        }
    }
    if (degree_bound > count * l) return KZG_ERR_INVALID_ARG;
    const size_t bound = degree_bound ? degree_bound : count * l;
    if (out_len != 0 && (eval_form ? out_len != n : (out_len < bound || out_len > n))) return KZG_ERR_INVALID_ARG;
    return recover_batch_size_check(blobs, count, n, l);
}
// ---- the serialized-form entries (kzg_recover_from_cosets_batch_bytes, kzg_retrieve_blobs_bytes) ---------------------------------------------
// A refused value is reported as (its index in the call) << 2 in one 32-bit word, the convention of the byte decoders, whose cap is the same
constexpr size_t RECOVER_BYTES_MAX_VALUES = (size_t)1 << 28;
// kzg_recover_from_cosets_batch_bytes: the table of kzg_recover_from_cosets_batch unchanged and in its order, then the cap on the values of a call
inline int32_t recover_bytes_check(bool any_null, const uint64_t* coset_indices, size_t index_rows, size_t blobs, size_t count, size_t n,
                                   size_t chunk_len, size_t degree_bound, bool eval_form, size_t out_len) {
    const int32_t rc = recover_batch_check(any_null, coset_indices, index_rows, blobs, count, n, chunk_len, degree_bound, eval_form, out_len);
    if (rc != KZG_OK) return rc;
    if (blobs > RECOVER_BYTES_MAX_VALUES / (count * chunk_len)) return KZG_ERR_TOO_LARGE;
    return KZG_OK;
}
// kzg_retrieve_blobs_bytes runs the same table first, then the verifier's (capi_coset.hip) on the blobs' chunks as its items: item i = b count + j has commitment row b and coset coset_indices[(index_rows == 1 ? 0 : b) count + j]
inline void retrieve_items(const uint64_t* coset_indices, size_t index_rows, size_t blobs, size_t count, std::vector<uint64_t>* cosets,
                           std::vector<uint64_t>* rows) {
    cosets->resize(blobs * count);
    rows->resize(blobs * count);
    for (size_t b = 0; b < blobs; ++b)
        for (size_t j = 0; j < count; ++j) {
            (*cosets)[b * count + j] = coset_indices[(index_rows == 1 ? 0 : b) * count + j];
            (*rows)[b * count + j] = b;
        }
}

// kzg_recover_batch_info's checks: the rows a shape alone can fail (no indices, no bound, no form: out_len is only held to <= n)
inline int32_t recover_batch_info_check(bool any_null, size_t blobs, size_t count, size_t n, size_t chunk_len, size_t out_len) {
    if (any_null || blobs == 0) return KZG_ERR_INVALID_ARG;
    const int32_t rc = recover_shape_check(count, n, chunk_len);
    if (rc != KZG_OK) return rc;
    if (out_len > n) return KZG_ERR_INVALID_ARG;
    return recover_batch_size_check(blobs, count, n, chunk_len);
}

// The grouping: a function of the shape and the budget alone.  A group is sized for its worst case, every blob with its own index row
// and its own pattern, so `group` blobs fit the budget whatever their indices; it holds at least one blob whatever the budget.
struct RecoverBatchGroups {
    size_t budget = 0;                     // the byte budget asked for (0 resolved to the default)
    size_t blob_bytes = 0;                 // device workspace per blob of a group
    size_t group = 1;                      // blobs per group (the last group of a call may hold fewer)
    size_t n_groups = 0;
    size_t group_bytes = 0;                // device workspace of one full group
};
inline RecoverBatchGroups recover_batch_groups(size_t blobs, size_t count, size_t n, size_t chunk_len, size_t group_bytes) {
    RecoverBatchGroups g;
    const size_t m = n / chunk_len, n_missing = m - count;
    const NttPlan np = ntt_plan(__builtin_ctzll(n), false, 256, 0);  // the byte counts depend on log n only
    const RecoverSplit sp = recover_vanish_split(m, n_missing, 1);   // a pattern never has more splits than the only one of a call
    g.budget = group_bytes ? group_bytes : RECOVER_GROUP_BYTES_DEFAULT;
    // work values | staged input, transform scratch, compacted rows | second transform scratch | item map, pattern, missing list, flag |
    // zdom, zsinv | partial products
    g.blob_bytes = n * 32 + n * 32 + np.bytes_tmp + 4 * (m + 1 + n_missing + 1) + 2 * 4 * RECOVER_LIMBS * m + (size_t)sp.splits * 4 * RECOVER_LIMBS * 2 * m;
    g.group = std::min(std::min(blobs, RECOVER_GROUP_MAX), std::max<size_t>(1, g.budget / g.blob_bytes));
    g.n_groups = (blobs + g.group - 1) / g.group;
    g.group_bytes = g.group * g.blob_bytes + 16;                     // + the alignment of the limb planes
    return g;
}

struct RecoverBatchPlan {
    size_t n = 0, l = 0, m = 0, count = 0, blobs = 0, index_rows = 0;
    int log_n = 0, log_l = 0, log_m = 0;
    size_t degree_bound = 0;               // resolved: 0 of the caller -> count l
    size_t out_len = 0;                    // resolved: 0 of the caller -> n
    bool eval_form = false;
    size_t n_missing = 0;                  // m - count: the length of every pattern
    size_t n_patterns = 0;                 // P <= index_rows distinct missing sets
    std::vector<uint32_t> missing;         // [pattern][n_missing], each ascending
    std::vector<uint32_t> item_of;         // [index row][coset] -> its item, RECOVER_NO_ITEM for a missing coset
    std::vector<uint32_t> pattern_of;      // [index row] -> its pattern, numbered in order of first appearance
    RecoverBatchGroups groups;
    // the word layout of rc[1] for a group, fixed by the shape, index_rows and groups.group (a ragged last group leaves gaps):
    // item_of rows x m | pattern_of group | missing patterns x |M| | flags group | (16-byte aligned) zdom patterns x 9 m | zsinv likewise |
    // partial patterns x splits x 9 x 2 m.  rows = patterns = 1 with one index row, else `group`.
    size_t w_item = 0, w_pat = 0, w_miss = 0, w_flag = 0, w_zdom = 0, w_zsinv = 0, w_part = 0, w_end = 0;
    size_t blob_pattern(size_t b) const { return pattern_of[index_rows == 1 ? 0 : b]; }
    // the items a blob HOLDS where the values lie (the stride between two blobs' values is held x l); 0: count, every held item is used.
    // recover_selected_plan sets it: count of the held items are used and item_of names positions below held
    size_t held = 0;
    size_t value_stride() const { return held ? held : count; }
};

inline void recover_batch_layout(RecoverBatchPlan* p) {
    const size_t cap = p->index_rows == 1 ? 1 : p->groups.group;     // index rows and patterns a group can hold
    const RecoverSplit sp = recover_vanish_split(p->m, p->n_missing, 1);
    p->w_item = 0;
    p->w_pat = p->w_item + cap * p->m;
    p->w_miss = p->w_pat + p->groups.group;
    p->w_flag = p->w_miss + cap * p->n_missing;
    p->w_zdom = (p->w_flag + p->groups.group + 3) & ~(size_t)3;
    p->w_zsinv = p->w_zdom + cap * RECOVER_LIMBS * p->m;
    p->w_part = p->w_zsinv + cap * RECOVER_LIMBS * p->m;
    p->w_end = p->w_part + cap * sp.splits * RECOVER_LIMBS * 2 * p->m;
}

// The plan of a call whose arguments passed recover_batch_check.  A blob's missing set depends on the SET of its indices only: each
// row's missing list comes out ascending, equal lists are one pattern; item_of stays per index row (the order may differ).  With one
// index row there is one pattern and no per-blob host work at all.
inline void recover_batch_plan(const uint64_t* coset_indices, size_t index_rows, size_t blobs, size_t count, size_t n, size_t chunk_len,
                               size_t degree_bound, bool eval_form, size_t out_len, size_t group_bytes, RecoverBatchPlan* plan) {
    RecoverBatchPlan& p = *plan;
    p = RecoverBatchPlan();
    p.n = n; p.l = chunk_len; p.m = n / chunk_len; p.count = count; p.blobs = blobs; p.index_rows = index_rows;
    p.log_n = __builtin_ctzll(n); p.log_l = __builtin_ctzll(chunk_len); p.log_m = p.log_n - p.log_l;
    p.degree_bound = degree_bound ? degree_bound : count * chunk_len;
    p.out_len = out_len ? out_len : n;
    p.eval_form = eval_form;
    p.n_missing = p.m - count;
    const size_t m = p.m;
    p.item_of.assign(index_rows * m, RECOVER_NO_ITEM);
    p.pattern_of.resize(index_rows);
    std::map<std::vector<uint32_t>, uint32_t> known;
    std::vector<uint32_t> row;
    for (size_t r = 0; r < index_rows; ++r) {
        uint32_t* item_of = p.item_of.data() + r * m;
        for (size_t i = 0; i < count; ++i) item_of[coset_indices[r * count + i]] = (uint32_t)i;
        row.clear();
        for (size_t k = 0; k < m; ++k)
            if (item_of[k] == RECOVER_NO_ITEM) row.push_back((uint32_t)k);
        const auto it = known.emplace(row, (uint32_t)known.size());
        if (it.second) p.missing.insert(p.missing.end(), row.begin(), row.end());
        p.pattern_of[r] = it.first->second;
    }
    p.n_patterns = known.size();
    p.groups = recover_batch_groups(blobs, count, n, chunk_len, group_bytes);
    recover_batch_layout(&p);
}

// The single call as a batch of one blob with one index row and one pattern
inline RecoverBatchPlan recover_batch_of_one(const RecoverPlan& one, bool eval_form) {
    RecoverBatchPlan p;
    p.n = one.n; p.l = one.l; p.m = one.m; p.count = one.count; p.blobs = 1; p.index_rows = 1;
    p.log_n = one.log_n; p.log_l = one.log_l; p.log_m = one.log_m;
    p.degree_bound = one.degree_bound;
    p.out_len = one.n;
    p.eval_form = eval_form;
    p.n_missing = one.missing.size();
    p.n_patterns = 1;
    p.missing = one.missing;
    p.item_of = one.item_of;
    p.pattern_of.assign(1, 0);
    p.groups = recover_batch_groups(1, one.count, one.n, one.l, 0);
    recover_batch_layout(&p);
    return p;
}

// What one upload carries for the blobs [b0, b0 + g) of the plan: the words [0, *words) of the layout -- the group's index rows, the
// pattern of each of its blobs renumbered within the group (order of first appearance), and those patterns' missing lists.  Returns
// the number of patterns of the group.
inline size_t recover_batch_stage(const RecoverBatchPlan& p, size_t b0, size_t g, std::vector<uint32_t>* stage, size_t* words) {
    stage->assign(p.w_flag, 0);
    uint32_t* s = stage->data();
    if (p.index_rows == 1) {
        std::copy(p.item_of.begin(), p.item_of.end(), s + p.w_item);
        std::copy(p.missing.begin(), p.missing.end(), s + p.w_miss);         // pattern_of: zeros
        *words = p.w_miss + p.n_missing;
        return 1;
    }
    std::copy(p.item_of.begin() + b0 * p.m, p.item_of.begin() + (b0 + g) * p.m, s + p.w_item);
    std::vector<uint32_t> local(p.n_patterns, RECOVER_NO_ITEM);
    size_t P = 0;
    for (size_t i = 0; i < g; ++i) {
        const uint32_t gp = p.pattern_of[b0 + i];
        if (local[gp] == RECOVER_NO_ITEM) {
            local[gp] = (uint32_t)P;
            std::copy(p.missing.begin() + gp * p.n_missing, p.missing.begin() + (gp + 1) * p.n_missing, s + p.w_miss + P * p.n_missing);
            ++P;
        }
        s[p.w_pat + i] = local[gp];
    }
    *words = p.w_miss + P * p.n_missing;
    return P;
}

// ---- kzg_retrieve_blobs_bytes_tolerant: a blob HOLDS `count` chunks and is recovered from the first use_count good ones ------------------
// The status of an item of that call (out_item_status); the decode refusals in the order the entries report them, a proof before a value
constexpr uint8_t RETRIEVE_ITEM_GOOD = 0, RETRIEVE_ITEM_BAD_EQUATION = 1, RETRIEVE_ITEM_PROOF_BYTES = 2, RETRIEVE_ITEM_PROOF_OFF_CURVE = 3,
                  RETRIEVE_ITEM_VALUE = 4;

// The host table of the call: that of kzg_retrieve_blobs_bytes's recovery half (recover_bytes_check) in its order, with the rows that speak of
// the cosets a blob is recovered FROM applied to use_count: 1 <= use_count <= count beside the range of count, the degree bound and out_len
// against use_count x l, the cost cap against m - use_count missing cosets.  The held indices are checked as before (below m, distinct per row).
inline int32_t retrieve_tolerant_check(bool any_null, const uint64_t* coset_indices, size_t index_rows, size_t blobs, size_t count, size_t use_count,
                                       size_t n, size_t chunk_len, size_t degree_bound, bool eval_form, size_t out_len) {
    if (any_null || blobs == 0) return KZG_ERR_INVALID_ARG;
    if (index_rows != 1 && index_rows != blobs) return KZG_ERR_INVALID_ARG;
    const int32_t rc = recover_shape_check(count, n, chunk_len);
    if (rc != KZG_OK) return rc;
    if (use_count == 0 || use_count > count) return KZG_ERR_INVALID_ARG;
    const size_t l = chunk_len, m = n / l;
    std::vector<uint64_t> seen((m + 63) / 64);
    for (size_t r = 0; r < index_rows; ++r) {
        std::fill(seen.begin(), seen.end(), 0);
        for (size_t i = 0; i < count; ++i) {
            const uint64_t k = coset_indices[r * count + i];
            if (k >= m) return KZG_ERR_INVALID_ARG;
            uint64_t& word = seen[k >> 6];
            const uint64_t bit = (uint64_t)1 << (k & 63);
            if (word & bit) return KZG_ERR_INVALID_ARG;
            word |= bit;
        }
    }
    if (degree_bound > use_count * l) return KZG_ERR_INVALID_ARG;
    const size_t bound = degree_bound ? degree_bound : use_count * l;
    if (out_len != 0 && (eval_form ? out_len != n : (out_len < bound || out_len > n))) return KZG_ERR_INVALID_ARG;
    const int32_t rs = recover_batch_size_check(blobs, use_count, n, l);
    if (rs != KZG_OK) return rs;
    if (blobs > RECOVER_BYTES_MAX_VALUES / (count * l)) return KZG_ERR_TOO_LARGE;
    return KZG_OK;
}

// The choice: blob b is recovered from its first use_count items of status RETRIEVE_ITEM_GOOD, in item order.  chosen: blobs x use_count
// positions below count, ascending per blob; blob_status[b] = 1 and the positions 0 .. use_count - 1 (never read: recover_selected_plan gives
// such a blob an empty item map) when the blob has fewer.  Returns the number of blobs that are not recovered.
inline size_t retrieve_choose(const uint8_t* item_status, size_t blobs, size_t count, size_t use_count, std::vector<uint32_t>* chosen,
                              std::vector<uint8_t>* blob_status) {
    chosen->resize(blobs * use_count);
    blob_status->assign(blobs, 0);
    size_t unrecovered = 0;
    for (size_t b = 0; b < blobs; ++b) {
        uint32_t* row = chosen->data() + b * use_count;
        size_t got = 0;
        for (size_t j = 0; j < count && got < use_count; ++j)
            if (item_status[b * count + j] == RETRIEVE_ITEM_GOOD) row[got++] = (uint32_t)j;
        if (got < use_count) {
            for (size_t j = 0; j < use_count; ++j) row[j] = (uint32_t)j;
            (*blob_status)[b] = 1;
            ++unrecovered;
        }
    }
    return unrecovered;
}

// The plan of the recovery from the chosen items, the values staying where the verifier's front end left them: `count` items per blob are held
// (plan.held), use_count of them are used (plan.count).  Patterns, missing lists, grouping and layout are those of recover_batch_plan on the
// chosen cosets as its rows; item_of names the position of a coset's item in the HELD layout, which is what k_recover_scatter indexes.  A blob
// of blob_status 1 gets an item map without items: no value of it is read, its work row is zero (the caller reports the zero row and flag 0).
// One index row for all blobs, every blob recovered and every blob with the same choice is planned as ONE row, as recover_batch_plan would be
// given it: one pattern, one upload, later groups reuse the first group's vanishing values.
inline void recover_selected_plan(const uint64_t* coset_indices, size_t index_rows, size_t blobs, size_t count, size_t use_count, const uint32_t* chosen,
                                  const uint8_t* blob_status, size_t n, size_t chunk_len, size_t degree_bound, bool eval_form, size_t out_len, size_t group_bytes,
                                  RecoverBatchPlan* plan) {
    bool one_row = index_rows == 1;
    for (size_t b = 0; b < blobs && one_row; ++b)
        one_row = !blob_status[b] && std::equal(chosen, chosen + use_count, chosen + b * use_count);
    const size_t rows = one_row ? 1 : blobs;
    std::vector<uint64_t> cosets(rows * use_count);
    for (size_t r = 0; r < rows; ++r)
        for (size_t j = 0; j < use_count; ++j) cosets[r * use_count + j] = coset_indices[(index_rows == 1 ? 0 : r) * count + chosen[r * use_count + j]];
    recover_batch_plan(cosets.data(), rows, blobs, use_count, n, chunk_len, degree_bound, eval_form, out_len, group_bytes, plan);
    plan->held = count;
    const size_t m = plan->m;
    for (size_t r = 0; r < rows; ++r) {
        uint32_t* item_of = plan->item_of.data() + r * m;
        for (size_t j = 0; j < use_count; ++j) item_of[cosets[r * use_count + j]] = blob_status[r] ? RECOVER_NO_ITEM : chosen[r * use_count + j];
    }
}

}  // namespace kzg
