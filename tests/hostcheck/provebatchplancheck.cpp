// tests/hostcheck/provebatchplancheck.cpp — TEST-ONLY driver for a plain g++ build (no GPU, no library) of the host side of the batched prover
// (csrc/host_prove_batch.h).  It checks
//   1. the argument table of kzg_compute_proof_batch row by row, and the status of one blob in the single call's order, every earlier row
//      winning over every later one, and that the first failing blob in index order is the one reported;
//   2. the length classes of mixed lengths: every blob in exactly one class or on the single list, the class of a blob the log2 of its padded
//      length, classes ascending, caller order kept inside a class; a blob over 2^12 elements on the single list; count = 0;
//   3. the groups of a class under a budget: never 0 rows, never more than the class, monotone in the budget, a budget of one byte gives groups of
//      one, the groups cover the class;
//   4. the packed layout of a group: offsets 32-byte aligned, ascending, each span the blob's whole elements, and the scatter of a group's rows
//      back to caller order: over all classes and groups together a permutation of the batched blobs (buffers of exactly the planned sizes).
// Built and run by tests/test_prove_batch_host.py, plain and under ASan + UBSan.  Exit status 1 and a line on stderr per violated check.
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_prove_batch.h"

using namespace kzg;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; fprintf(stderr, "provebatchplancheck: line %d: %s\n", __LINE__, #c); } } while (0)

static void check_order() {
    bool done = true;
    const size_t SRS = 3000;
    CHECK(prove_batch_check_polys(false, false, 512, 4, SRS, &done) == KZG_OK && !done);
    CHECK(prove_batch_check_polys(true, true, 3, 0, 0, &done) == KZG_ERR_INVALID_ARG && !done);                 // row 1 in front of everything
    CHECK(prove_batch_check_polys(false, true, 3, 0, SRS, &done) == KZG_OK && done);                            // count = 0 in front of the data and the length
    CHECK(prove_batch_check_polys(false, true, 3, 1, SRS, &done) == KZG_ERR_INVALID_ARG && !done);               // the data in front of the length
    CHECK(prove_batch_check_polys(false, false, 0, 1, SRS, &done) == KZG_ERR_INVALID_INPUT_LENGTH);
    CHECK(prove_batch_check_polys(false, false, 48, 1, SRS, &done) == KZG_ERR_INVALID_INPUT_LENGTH);
    CHECK(prove_batch_check_polys(false, false, (size_t)3 << 30, 1, SRS, &done) == KZG_ERR_INVALID_INPUT_LENGTH);  // no power of two in front of too large
    CHECK(prove_batch_check_polys(false, false, (size_t)1 << 29, 1, SRS, &done) == KZG_ERR_TOO_LARGE);           // too large in front of the SRS
    CHECK(prove_batch_check_polys(false, false, 512, ((size_t)1 << 31) + 1, SRS, &done) == KZG_ERR_TOO_LARGE);
    CHECK(prove_batch_check_polys(false, false, 512, (size_t)1 << 31, SRS, &done) == KZG_OK);
    CHECK(prove_batch_check_polys(false, false, 4096, 1, SRS, &done) == KZG_ERR_SRS_CAPACITY_EXCEEDED);
    CHECK(prove_batch_check_polys(false, false, 2048, 1, SRS, &done) == KZG_OK);
    // one blob: null bytes, too large, off the curve, empty, beyond the SRS -- each in front of the ones after it
    const size_t HUGE_LEN = (((size_t)1 << 28) + 1) * 32;
    CHECK(prove_batch_blob_status(false, 1000, false, SRS) == KZG_OK);
    CHECK(prove_batch_blob_status(true, HUGE_LEN, true, 1) == KZG_ERR_INVALID_ARG);
    CHECK(prove_batch_blob_status(true, 0, false, SRS) == KZG_ERR_ZERO_LENGTH);                                 // no length: no bytes are needed
    CHECK(prove_batch_blob_status(false, HUGE_LEN, true, 1) == KZG_ERR_TOO_LARGE);
    CHECK(prove_batch_blob_status(false, HUGE_LEN - 32, false, SIZE_MAX) == KZG_OK);
    CHECK(prove_batch_blob_status(false, 0, true, 1) == KZG_ERR_G1_NOT_ON_CURVE);
    CHECK(prove_batch_blob_status(false, 4096 * 32, true, SRS) == KZG_ERR_G1_NOT_ON_CURVE);
    CHECK(prove_batch_blob_status(false, 0, false, 0) == KZG_ERR_ZERO_LENGTH);
    CHECK(prove_batch_blob_status(false, 2049 * 32, false, SRS) == KZG_ERR_SRS_CAPACITY_EXCEEDED);              // padded to 4096
    CHECK(prove_batch_blob_status(false, 2048 * 32, false, SRS) == KZG_OK);
    CHECK(prove_batch_blob_status(false, 2048 * 32 + 1, false, SRS) == KZG_ERR_SRS_CAPACITY_EXCEEDED);
    CHECK(prove_batch_blob_status(false, 31, false, 1) == KZG_OK);
    CHECK(prove_batch_blob_status(false, 33, false, 1) == KZG_ERR_SRS_CAPACITY_EXCEEDED);
    // the first failing blob in index order
    const int32_t st[8] = {KZG_OK, KZG_OK, KZG_OK, KZG_ERR_G1_NOT_ON_CURVE, KZG_OK, KZG_ERR_ZERO_LENGTH, KZG_OK, KZG_ERR_INVALID_ARG};
    size_t bad = 77;
    CHECK(prove_batch_first_failure(st, 3, &bad) == KZG_OK && bad == 77);
    CHECK(prove_batch_first_failure(st, 8, &bad) == KZG_ERR_G1_NOT_ON_CURVE && bad == 3);
    CHECK(prove_batch_first_failure(st + 4, 4, &bad) == KZG_ERR_ZERO_LENGTH && bad == 1);
    CHECK(prove_batch_first_failure(st, 8, nullptr) == KZG_ERR_G1_NOT_ON_CURVE);
    CHECK(prove_batch_first_failure(st, 0, &bad) == KZG_OK && bad == 1);
}

static void check_plan(const std::vector<size_t>& lens, const std::vector<size_t>& budgets) {
    const size_t count = lens.size();
    const ProveBatchPlan p = prove_batch_plan(lens.data(), count);
    std::vector<int> seen(count, 0);
    int last_log = -1;
    size_t at = 0;
    for (const ProveBatchClass& c : p.classes) {
        CHECK(c.log_n > last_log && c.log_n <= PROVE_BATCH_MAX_LOG && c.count > 0 && c.first == at);
        last_log = c.log_n;
        at += c.count;
        for (size_t k = 0; k < c.count; ++k) {
            const size_t i = p.order[c.first + k];
            CHECK(i < count);
            if (i >= count) continue;
            ++seen[i];
            const size_t elems = (lens[i] + 31) / 32;
            CHECK(((size_t)1 << c.log_n) >= elems && (c.log_n == 0 || ((size_t)1 << (c.log_n - 1)) < elems));
            if (k) CHECK(p.order[c.first + k - 1] < i);                                      // caller order inside a class
        }
    }
    CHECK(at == p.order.size());
    for (size_t k = 0; k < p.single.size(); ++k) {
        const size_t i = p.single[k];
        CHECK(i < count);
        if (i >= count) continue;
        ++seen[i];
        CHECK((lens[i] + 31) / 32 > ((size_t)1 << PROVE_BATCH_MAX_LOG));
        if (k) CHECK(p.single[k - 1] < i);
    }
    for (size_t i = 0; i < count; ++i) CHECK(seen[i] == 1);
    // groups, packing and scatter per budget
    for (size_t budget : budgets) {
        std::vector<uint64_t> out(count * 8, 0);
        std::vector<uint8_t> out_b(count, 0);
        for (const ProveBatchClass& c : p.classes) {
            const size_t n = (size_t)1 << c.log_n;
            const size_t group = prove_batch_group_rows(n, c.count, budget, true);
            CHECK(group >= 1 && group <= c.count && group <= PROVE_GROUP_ROWS_MAX);
            CHECK(group == 1 || group * prove_batch_row_bytes(n, true) <= (budget ? budget : PROVE_GROUP_BYTES_DEFAULT));
            if (budget == 1) CHECK(group == 1);
            CHECK(prove_batch_group_rows(n, c.count, budget, false) >= group);                // rows without packed bytes are smaller
            if (budget) CHECK(prove_batch_group_rows(n, c.count, 2 * budget, true) >= group); // monotone
            size_t covered = 0, groups = 0;
            for (size_t g0 = 0; g0 < c.count; g0 += group, ++groups) {
                const size_t rows = std::min(group, c.count - g0);
                const size_t* order = p.order.data() + c.first + g0;
                std::vector<size_t> offs(rows + 1);
                prove_batch_pack_offsets(lens.data(), order, rows, offs.data());
                CHECK(offs[0] == 0);
                for (size_t r = 0; r < rows; ++r) {
                    CHECK(offs[r] % 32 == 0 && offs[r + 1] - offs[r] == (lens[order[r]] + 31) / 32 * 32 && offs[r + 1] - offs[r] <= n * 32);
                }
                std::vector<uint8_t> packed(offs[rows], 0xEE);                               // exactly the planned size: the packer's writes are checked accesses
                for (size_t r = 0; r < rows; ++r) {
                    const size_t len = lens[order[r]], span = offs[r + 1] - offs[r];
                    if (len) memset(packed.data() + offs[r], 0x11, len);
                    if (span > len) memset(packed.data() + offs[r] + len, 0, span - len);
                }
                std::vector<uint64_t> res(rows * 8);
                std::vector<uint8_t> res_b(rows);
                for (size_t r = 0; r < rows; ++r) { for (int w = 0; w < 8; ++w) res[r * 8 + w] = (order[r] + 1) * 100 + w; res_b[r] = (uint8_t)(order[r] % 251 + 1); }
                prove_batch_scatter(res.data(), order, rows, 8, out.data());
                prove_batch_scatter_bytes(res_b.data(), order, rows, out_b.data());
                prove_batch_scatter(res.data(), order, rows, 8, nullptr);                    // an output the caller left out
                prove_batch_scatter(nullptr, order, rows, 8, out.data());
                covered += rows;
            }
            CHECK(covered == c.count && groups == prove_batch_groups(c.count, group));
        }
        for (size_t i = 0; i < count; ++i) {                                                // a permutation: every batched row written once, with its own values
            const bool batched = (lens[i] + 31) / 32 <= ((size_t)1 << PROVE_BATCH_MAX_LOG);
            for (int w = 0; w < 8; ++w) CHECK(out[i * 8 + w] == (batched ? (i + 1) * 100 + w : 0));
            CHECK(out_b[i] == (batched ? (uint8_t)(i % 251 + 1) : 0));
        }
    }
}

int main() {
    check_order();
    const std::vector<size_t> budgets = {0, 1, 100, 4096, 100000, (size_t)1 << 20, (size_t)1 << 30};
    check_plan({}, budgets);                                                                 // count = 0
    check_plan({31}, budgets);
    check_plan({31, 32, 33, 1000, 1399, 4096 * 32, 4096 * 32 + 1, 4097 * 32, 64, 65, 2048 * 32, 1, 32 * 3, 32 * 5, 1000, 1000, 999}, budgets);
    std::vector<size_t> many;
    for (size_t i = 0; i < 700; ++i) many.push_back(1 + (i * 7919) % (5000 * 32));          // every class and the single list
    check_plan(many, budgets);
    std::vector<size_t> same(1030, 512 * 32);
    check_plan(same, budgets);
    if (failures) { fprintf(stderr, "provebatchplancheck: %d failures\n", failures); return 1; }
    printf("prove batch plan ok\n");
    return 0;
}
