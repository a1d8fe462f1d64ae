// tests/hostcheck/recoverbytescheck.cpp — TEST-ONLY stand-alone program: the host-visible pieces of the retriever's serialized form.
//   1. fr_encode_wire_to_be (csrc/g1_decode.h), compiled by g++ with -DKZG_BOUND_CHECK (every lazy-reduction bound aborts): the exact inverse
//      of fr_decode_be_to_wire on 0, 1, r - 1, 2^253 and 10^4 random canonical values, and equal to kzg_host::fr_wire_to_canonical plus a
//      byte reversal (a second implementation, 64-bit Montgomery words).
//   2. the argument checks of kzg_recover_from_cosets_batch_bytes / kzg_retrieve_blobs_bytes (csrc/host_recover.h: recover_bytes_check),
//      walked through every row of the table in its order, and retrieve_items.
// Run by tests/test_recover_bytes_host.py, once as it is and once under -fsanitize=address,undefined.  Prints "recoverbytescheck ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "g1_decode.h"
#include "host_fr.h"
#include "host_recover.h"

using namespace kzg;
namespace H = kzg_host;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (++failures <= 20) { fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static uint64_t rng_state = 0x243F6A8885A308D3ULL;
static uint64_t next64() {                         // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

static void be32_of_plain(uint8_t out[32], const uint64_t w[4]) {
    for (int i = 0; i < 4; ++i)
        for (int b = 0; b < 8; ++b) out[8 * i + b] = (uint8_t)(w[3 - i] >> (8 * (7 - b)));
}

// plain: a canonical integer below r
static void check_round_trip(const uint64_t plain[4]) {
    uint8_t b[32], back[32];
    be32_of_plain(b, plain);
    uint32_t raw[8], wire[8], out_raw[8];
    g1_bytes_to_words(raw, b);
    EXPECT(fr_decode_be_to_wire(wire, raw), "a canonical value is refused");
    fr_encode_wire_to_be(out_raw, wire);
    memcpy(back, out_raw, 32);                     // the kernel stores the words as they are: little-endian words of the byte string
    EXPECT(memcmp(back, b, 32) == 0, "encode(decode(bytes)) is not the identity at %016llx..", (unsigned long long)plain[3]);
    // the second implementation: 64-bit Montgomery words -> canonical words, reversed
    uint64_t w64[4], canon[4];
    memcpy(w64, wire, 32);
    H::fr_wire_to_canonical(w64, canon);
    uint8_t rev[32];
    be32_of_plain(rev, canon);
    EXPECT(memcmp(canon, plain, 32) == 0, "the decoded wire words are not the Montgomery form of the integer");
    EXPECT(memcmp(back, rev, 32) == 0, "fr_encode_wire_to_be differs from fr_wire_to_canonical + byte reversal");
    // ... and decode(encode(wire)) on the wire side
    uint32_t again[8];
    EXPECT(fr_decode_be_to_wire(again, out_raw) && memcmp(again, wire, 32) == 0, "decode(encode(wire)) is not the identity");
}

static void check_codec() {
    const uint64_t* r = H::FR_MODULUS_WORDS;
    const uint64_t zero[4] = {0, 0, 0, 0}, one[4] = {1, 0, 0, 0}, r_minus_1[4] = {r[0] - 1, r[1], r[2], r[3]}, two253[4] = {0, 0, 0, (uint64_t)1 << 61};
    check_round_trip(zero);
    check_round_trip(one);
    check_round_trip(r_minus_1);
    check_round_trip(two253);                      // 2^253 < r < 2^254
    for (int i = 0; i < 10000; ++i) {
        uint64_t v[4] = {next64(), next64(), next64(), next64() >> 2};           // < 2^254
        while (v[3] >= r[3]) v[3] = next64() >> 2;                              // top word below r's: below r
        check_round_trip(v);
    }
    // the refusals the decoder keeps: r, r + 1, 2^256 - 1
    const uint64_t bad[3][4] = {{r[0], r[1], r[2], r[3]}, {r[0] + 1, r[1], r[2], r[3]}, {~0ULL, ~0ULL, ~0ULL, ~0ULL}};
    for (const auto& v : bad) {
        uint8_t b[32];
        be32_of_plain(b, v);
        uint32_t raw[8], wire[8];
        g1_bytes_to_words(raw, b);
        EXPECT(!fr_decode_be_to_wire(wire, raw), "a value not below r is accepted");
    }
}

// ---- the table of kzg_recover_from_cosets_batch_bytes, in its order ------------------------------------------------------------------------
static void check_table() {
    const size_t n = 64, l = 4, m = n / l, B = 3, count = 5;
    const uint64_t ks[B * count] = {3, 0, 9, 14, 5, 1, 2, 3, 4, 5, 15, 0, 7, 8, 2};
    auto call = [&](bool any_null, const uint64_t* idx, size_t rows, size_t blobs, size_t cnt, size_t n_, size_t l_, size_t bound, bool form, size_t out_len) {
        return recover_bytes_check(any_null, idx, rows, blobs, cnt, n_, l_, bound, form, out_len);
    };
    EXPECT(call(false, ks, B, B, count, n, l, 0, false, 0) == KZG_OK, "a valid call is refused");
    EXPECT(call(false, ks, 1, B, count, n, l, 0, true, n) == KZG_OK, "a valid call with one index row is refused");
    EXPECT(call(true, ks, 2, B, count, 0, l, 0, false, 0) == KZG_ERR_INVALID_ARG, "1. a null pointer in front of everything");
    EXPECT(call(false, ks, 1, 0, count, 0, l, 0, false, 0) == KZG_ERR_INVALID_ARG, "1. blobs = 0 in front of n = 0");
    EXPECT(call(false, ks, 2, B, count, 0, l, 0, false, 0) == KZG_ERR_INVALID_ARG, "2. index_rows neither 1 nor blobs, in front of n = 0");
    EXPECT(call(false, ks, B, B, count, 0, l, 0, false, 0) == KZG_ERR_NOT_POWER_OF_TWO, "3. n = 0");
    EXPECT(call(false, ks, B, B, count, 96, 3, 0, false, 0) == KZG_ERR_NOT_POWER_OF_TWO, "3. n = 96 in front of l = 3");
    EXPECT(call(false, ks, B, B, count, (size_t)1 << 25, 3, 0, false, 0) == KZG_ERR_DOMAIN, "3. n = 2^25 in front of l = 3");
    EXPECT(call(false, ks, B, B, count, 1, 1, 0, false, 0) == KZG_ERR_INVALID_ARG, "3. n = 1");
    EXPECT(call(false, ks, B, B, count, n, 0, 0, false, 0) == KZG_ERR_INVALID_ARG && call(false, ks, B, B, count, n, 3, 0, false, 0) == KZG_ERR_INVALID_ARG &&
           call(false, ks, B, B, count, n, 64, 0, false, 0) == KZG_ERR_INVALID_ARG, "3. the chunk length");
    EXPECT(call(false, ks, B, B, 0, n, l, 0, false, 0) == KZG_ERR_INVALID_ARG && call(false, ks, B, B, m + 1, n, l, 0, false, 0) == KZG_ERR_INVALID_ARG, "3. count");
    uint64_t bad[B * count];
    memcpy(bad, ks, sizeof ks);
    bad[2 * count + 1] = m;
    EXPECT(call(false, bad, B, B, count, n, l, 99, false, 0) == KZG_ERR_INVALID_ARG, "4. an index = m in the last row");
    memcpy(bad, ks, sizeof ks);
    bad[count + 4] = 1;
    EXPECT(call(false, bad, B, B, count, n, l, 0, false, 0) == KZG_ERR_INVALID_ARG, "4. a duplicate in the middle row");
    EXPECT(call(false, bad, 1, B, count, n, l, 0, false, 0) == KZG_OK, "4. with one index row only the first row is read");
    EXPECT(call(false, ks, B, B, count, n, l, count * l + 1, false, 1) == KZG_ERR_INVALID_ARG, "5. too few cosets, in front of out_len");
    EXPECT(call(false, ks, B, B, count, n, l, 0, false, count * l - 1) == KZG_ERR_INVALID_ARG && call(false, ks, B, B, count, n, l, 0, false, n + 1) == KZG_ERR_INVALID_ARG &&
           call(false, ks, B, B, count, n, l, 0, true, n - 1) == KZG_ERR_INVALID_ARG, "6. out_len");
    EXPECT(call(false, ks, B, B, count, n, l, 8, false, 8) == KZG_OK && call(false, ks, B, B, count, n, l, 8, false, 7) == KZG_ERR_INVALID_ARG, "6. out_len against the bound");
    const uint64_t zero_idx[1] = {0};
    EXPECT(call(false, zero_idx, 1, 1, 1, (size_t)1 << 24, 1, 0, false, 0) == KZG_ERR_TOO_LARGE, "7. the cost cap of one blob");
    EXPECT(call(false, zero_idx, 1, 1, 1, (size_t)1 << 24, 1, 0, true, 2) == KZG_ERR_INVALID_ARG, "6 in front of 7");
    EXPECT(call(false, ks, 1, SIZE_MAX / (n * 32) + 1, count, n, l, 0, false, 0) == KZG_ERR_INVALID_ARG, "8. the batch's arrays overflow size_t");
    // 9. the cap on the values of a call: 2^28, the last row of the table (an index row of 2^10 cosets of 2^10 values: 2^20 per blob)
    {
        const size_t cn = (size_t)1 << 20, cl = (size_t)1 << 10, cm = cn / cl;
        std::vector<uint64_t> all(cm);
        for (size_t i = 0; i < cm; ++i) all[i] = i;
        EXPECT(call(false, all.data(), 1, 256, cm, cn, cl, 0, false, 0) == KZG_OK, "9. 2^28 values pass");
        EXPECT(call(false, all.data(), 1, 257, cm, cn, cl, 0, false, 0) == KZG_ERR_TOO_LARGE, "9. more than 2^28 values");
        EXPECT(call(false, all.data(), 1, 257, cm, cn, cl, 0, true, 5) == KZG_ERR_INVALID_ARG, "6 in front of 9");
        EXPECT(recover_batch_check(false, all.data(), 1, 257, cm, cn, cl, 0, false, 0) == KZG_OK, "row 9 belongs to the serialized entries only");
    }
    // the blobs' chunks as the verifier's items
    std::vector<uint64_t> cosets, rows;
    retrieve_items(ks, B, B, count, &cosets, &rows);
    EXPECT(cosets.size() == B * count && rows.size() == B * count, "retrieve_items: sizes");
    for (size_t i = 0; i < B * count; ++i) EXPECT(cosets[i] == ks[i] && rows[i] == i / count, "retrieve_items: item %zu", i);
    retrieve_items(ks + count, 1, B, count, &cosets, &rows);
    for (size_t i = 0; i < B * count; ++i) EXPECT(cosets[i] == ks[count + i % count] && rows[i] == i / count, "retrieve_items, one row: item %zu", i);
}

int main() {
    check_codec();
    check_table();
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    printf("recoverbytescheck ok\n");
    return 0;
}
