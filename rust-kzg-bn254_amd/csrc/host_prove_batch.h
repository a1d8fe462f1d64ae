// host_prove_batch.h -- the host side of the batched prover (kzg_compute_proof_batch, kzg_compute_blob_proof_batch,
// kzg_commit_and_prove_blob_batch; capi_provebatch.hip, provebatch.hip): the argument checks in their fixed order, the status of one blob in
// the single call's order, the sorting of blobs into length classes (one per log2 of the padded length), the groups a class is worked through
// under a byte budget, the layout of a group's packed bytes, and the scatter of a group's rows back to the caller's order.  Pure host code: no
// HIP type, no kzg_ctx; also compiled with g++ by tests/hostcheck/provebatchplancheck.cpp (plain and under ASan + UBSan).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/kzg_bn254_mi355x.h"

namespace kzg {

constexpr int PROVE_BATCH_MAX_LOG = 12;                               // the fused kernel's largest class (PB_MAX_LOG of provebatch_lanes.h)
constexpr size_t PROVE_BATCH_MAX_ELEMS = (size_t)1 << 28;             // polynomial.rs:42-46
constexpr size_t PROVE_GROUP_BYTES_DEFAULT = (size_t)256 << 20;       // device workspace of a group; kzg_ctx_set_prove_group_bytes overrides it
constexpr size_t PROVE_GROUP_ROWS_MAX = (size_t)1 << 20;              // rows of a launch (the blob is blockIdx.x)
constexpr size_t PROVE_ROW_SMALL_BYTES = 16 + 32 + 32 + 128;          // per row: descriptor, z, y, the prep record

inline size_t prove_batch_next_pow2(size_t x) { size_t p = 1; while (p < x) p <<= 1; return p; }   // next_power_of_two(0) == 1
inline int prove_batch_log2(size_t n) { int l = 0; while (((size_t)1 << l) < n) ++l; return l; }

// kzg_compute_proof_batch(_device), in this order:
//   1  a null handle, an SRS of another context, no output for the proofs                      KZG_ERR_INVALID_ARG
//   2  count = 0                                                                               KZG_OK, nothing written
//   3  no evaluations or no points                                                             KZG_ERR_INVALID_ARG
//   4  n = 0 or no power of two                       (helpers.rs:485-487)                     KZG_ERR_INVALID_INPUT_LENGTH
//   5  n > 2^28, count x n beyond 2^40                (polynomial.rs:42-46)                    KZG_ERR_TOO_LARGE
//   6  n > the SRS                                    (kzg.rs:89-94, the quotient's commitment) KZG_ERR_SRS_CAPACITY_EXCEEDED
// `done` is set when the call has nothing more to do (row 2).
inline int32_t prove_batch_check_polys(bool bad_handles, bool no_data, size_t n, size_t count, size_t srs_len, bool* done) {
    *done = false;
    if (bad_handles) return KZG_ERR_INVALID_ARG;
    if (count == 0) { *done = true; return KZG_OK; }
    if (no_data) return KZG_ERR_INVALID_ARG;
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_INVALID_INPUT_LENGTH;
    if (n > PROVE_BATCH_MAX_ELEMS || count > ((size_t)1 << 40) / n) return KZG_ERR_TOO_LARGE;
    if (n > srs_len) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    return KZG_OK;
}

// One blob of the bytes entries, in the single call's order (kzg_compute_blob_proof / kzg_commit_and_prove_blob):
//   a length without bytes                                                                      KZG_ERR_INVALID_ARG
//   more than 2^28 elements                           (polynomial.rs:42-46)                    KZG_ERR_TOO_LARGE
//   a commitment that is not on the curve             (kzg.rs:295)                             KZG_ERR_G1_NOT_ON_CURVE
//   an empty blob                                     (helpers.rs:554-558: no domain of it)    KZG_ERR_ZERO_LENGTH
//   a padded length beyond the SRS                    (kzg.rs:89-94)                           KZG_ERR_SRS_CAPACITY_EXCEEDED
// The single calls compare the padded length with the caller's roots (kzg.rs:135-139) where this table has the empty blob: a batch of mixed
// lengths has no one roots array, and the roots of an empty blob cannot exist.
inline int32_t prove_batch_blob_status(bool null_bytes, size_t len, bool commitment_off_curve, size_t srs_len) {
    if (len && null_bytes) return KZG_ERR_INVALID_ARG;
    const size_t elems = len / 32 + (len % 32 != 0);
    if (elems > PROVE_BATCH_MAX_ELEMS) return KZG_ERR_TOO_LARGE;
    if (commitment_off_curve) return KZG_ERR_G1_NOT_ON_CURVE;
    if (len == 0) return KZG_ERR_ZERO_LENGTH;
    if (prove_batch_next_pow2(elems) > srs_len) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    return KZG_OK;
}
// the first failing blob in index order: its status, its index into *bad (untouched when every blob passes or bad is null)
inline int32_t prove_batch_first_failure(const int32_t* status, size_t count, size_t* bad) {
    for (size_t i = 0; i < count; ++i)
        if (status[i] != KZG_OK) { if (bad) *bad = i; return status[i]; }
    return KZG_OK;
}

// ---- classes -----------------------------------------------------------------------------------------------------------------------------------
struct ProveBatchClass { int log_n; size_t first, count; };          // order[first .. first + count) are the class's blobs, in caller order
struct ProveBatchPlan {
    std::vector<size_t> order;                                       // caller indices: the classes one after the other, then nothing else
    std::vector<ProveBatchClass> classes;                            // ascending log_n <= PROVE_BATCH_MAX_LOG
    std::vector<size_t> single;                                      // blobs of more than 2^PROVE_BATCH_MAX_LOG elements, in caller order: the single-proof path
};
// lens: byte lengths, every one of them > 0 with at most 2^28 elements (prove_batch_blob_status)
inline ProveBatchPlan prove_batch_plan(const size_t* lens, size_t count) {
    ProveBatchPlan p;
    size_t per[PROVE_BATCH_MAX_LOG + 1] = {};
    std::vector<int> lg(count);
    for (size_t i = 0; i < count; ++i) {
        const size_t elems = lens[i] / 32 + (lens[i] % 32 != 0);
        lg[i] = prove_batch_log2(prove_batch_next_pow2(elems));
        if (lg[i] > PROVE_BATCH_MAX_LOG) p.single.push_back(i); else ++per[lg[i]];
    }
    size_t at[PROVE_BATCH_MAX_LOG + 1], first = 0;
    for (int l = 0; l <= PROVE_BATCH_MAX_LOG; ++l) {
        at[l] = first;
        if (per[l]) p.classes.push_back(ProveBatchClass{l, first, per[l]});
        first += per[l];
    }
    p.order.resize(first);
    for (size_t i = 0; i < count; ++i)
        if (lg[i] <= PROVE_BATCH_MAX_LOG) p.order[at[lg[i]]++] = i;
    return p;
}

// ---- groups ------------------------------------------------------------------------------------------------------------------------------------
// device bytes of one row of a class of n evaluations: the row, its quotient row, the small records, and (bytes entries) its packed bytes
inline size_t prove_batch_row_bytes(size_t n, bool from_bytes) { return n * 32 * (from_bytes ? 3 : 2) + PROVE_ROW_SMALL_BYTES; }
// rows per group under the budget (0: the default): never 0, never more than the class or a launch takes.  The groups are as large as the
// budget allows and the last one takes the rest: equal groups were measured and gave no gain at 4 096 rows of 1 024 .. 4 096 evaluations
// (0.6-4 % slower across sessions that differ by 2 % themselves; profiles/prove_batch.md section 6)
inline size_t prove_batch_group_rows(size_t n, size_t count, size_t budget, bool from_bytes) {
    if (budget == 0) budget = PROVE_GROUP_BYTES_DEFAULT;
    const size_t rows = budget / prove_batch_row_bytes(n, from_bytes);
    return std::max<size_t>(1, std::min(std::min(rows, count), PROVE_GROUP_ROWS_MAX));
}
inline size_t prove_batch_groups(size_t count, size_t group_rows) { return (count + group_rows - 1) / group_rows; }

// ---- the packed bytes of a group ---------------------------------------------------------------------------------------------------------------
// blob r of the group at offs[r], 32-byte aligned, zero-filled up to its last whole element: offs has rows + 1 entries, offs[rows] the total
inline void prove_batch_pack_offsets(const size_t* lens, const size_t* order, size_t rows, size_t* offs) {
    size_t off = 0;
    for (size_t r = 0; r < rows; ++r) {
        offs[r] = off;
        const size_t len = lens[order[r]];
        off += (len / 32 + (len % 32 != 0)) * 32;
    }
    offs[rows] = off;
}

// ---- scatter -----------------------------------------------------------------------------------------------------------------------------------
// row r of a group's result (words 64-bit words per row) to row order[r] of the caller's array; either may be null
inline void prove_batch_scatter(const uint64_t* group_rows, const size_t* order, size_t rows, size_t words, uint64_t* out) {
    if (!group_rows || !out) return;
    for (size_t r = 0; r < rows; ++r)
        for (size_t w = 0; w < words; ++w) out[order[r] * words + w] = group_rows[r * words + w];
}
inline void prove_batch_scatter_bytes(const uint8_t* group_rows, const size_t* order, size_t rows, uint8_t* out) {
    if (!group_rows || !out) return;
    for (size_t r = 0; r < rows; ++r) out[order[r]] = group_rows[r];
}

}  // namespace kzg
