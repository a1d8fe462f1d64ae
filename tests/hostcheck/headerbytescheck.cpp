// tests/hostcheck/headerbytescheck.cpp — TEST-ONLY stand-alone program (its own main; tests/test_header_bytes_host.py builds it once
// plainly and once with -fsanitize=address,undefined) over the host-compilable code of the serialized blob headers:
//   * csrc/header_item_stream.h, the block producer a lane of k_header_item_digests runs, compiled by g++ with -DKZG_BOUND_CHECK (every
//     lazy-reduction bound is an abort): for each header all six blocks against the item message of host_fiat_shamir.h
//     (header_item_message, padded by hand) and the digest against host_sha256.h.  The producer reads what the kernel reads: the
//     commitment as the gnark bytes of host_coset_bytes.h g1_encode_be, the G2 elements in the device format (g2_affine_wire_to_device).
//     Cases: random multiples of the generators; a commitment and its negative (both y signs); each of the three elements as the
//     identity, alone and all together; coordinates with leading zero bytes (found by search: a top byte of zero).
//   * csrc/host_header_bytes.h g2_encode_be: the bytes decode back to the point with host_g2_decode.h (the generator excepted, which
//     that decoder refuses by rule), both flags occur, the identity is 0x40 and 63 zeros, a coordinate not below p is refused.
// Prints "headerbytescheck ok <headers> <leading-zero coordinates>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "curve_g2.h"
#include "header_item_stream.h"
#include "host_fiat_shamir.h"
#include "host_header_bytes.h"

namespace H = kzg_host;

#define CHECK(cond) do { if (!(cond)) { printf("headerbytescheck: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int n_headers = 0, n_leading_zero = 0, n_flag[2] = {0, 0};

static bool top_byte_zero(const uint64_t mont[4]) {
    H::Fq a;
    memcpy(a.l, mont, 32);
    return (H::fq_to_plain(a).l[3] >> 56) == 0;
}

// one header through both producers
static int check_header(uint64_t d, const uint64_t c[8], const uint64_t c2[16], const uint64_t pi2[16]) {
    uint8_t item[H::HEADER_ITEM_BYTES + 64];
    memset(item, 0, sizeof item);
    H::header_item_message(d, c, c2, pi2, item);
    item[H::HEADER_ITEM_BYTES] = 0x80;
    H::put_u64be(item + sizeof item - 8, (uint64_t)H::HEADER_ITEM_BYTES * 8);
    uint8_t want[32];
    {
        H::Sha256 sh;
        H::sha256_init(sh);
        H::sha256_update(sh, item, H::HEADER_ITEM_BYTES);
        H::sha256_final(sh, want);
    }
    alignas(16) uint8_t c_be[32];
    alignas(16) uint32_t dev[2][32];
    CHECK(H::g1_encode_be(c, c_be));
    kzg::g2_affine_wire_to_device(dev[0], reinterpret_cast<const uint32_t*>(c2), nullptr);
    kzg::g2_affine_wire_to_device(dev[1], reinterpret_cast<const uint32_t*>(pi2), nullptr);
    alignas(16) uint32_t c_words[8];
    memcpy(c_words, c_be, 32);                                         // (what a little-endian load of the bytes leaves)
    kzg::HeaderItemSrc src;
    src.commitment_be = c_words; src.c2 = dev[0]; src.pi2 = dev[1]; src.d = d;
    CHECK(kzg::HEADER_ITEM_BLOCKS * 64 == sizeof item);
    for (uint32_t b = 0; b < kzg::HEADER_ITEM_BLOCKS; ++b) {
        uint32_t w[16];
        kzg::header_item_block(w, src, b);
        for (int j = 0; j < 16; ++j) {
            const uint8_t* p = item + 64 * b + 4 * j;
            const uint32_t be = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
            if (w[j] != be) { printf("headerbytescheck: header %d block %u word %d: %08x, the host message has %08x\n", n_headers, b, j, w[j], be); return 1; }
        }
    }
    uint32_t dig[8];
    kzg::header_item_digest(dig, src);
    CHECK(memcmp(dig, want, 32) == 0);
    ++n_headers;
    for (int q = 0; q < 2; ++q) if (top_byte_zero(c + 4 * q)) ++n_leading_zero;
    for (int q = 0; q < 4; ++q) { if (top_byte_zero(c2 + 4 * q)) ++n_leading_zero; if (top_byte_zero(pi2 + 4 * q)) ++n_leading_zero; }
    return 0;
}

static int check_encoder(const uint64_t wire[16], bool is_generator) {
    uint8_t b[64];
    CHECK(H::g2_encode_be(wire, b));
    const H::G2 p = H::g2_from_wire(wire);
    if (p.inf) {
        CHECK(b[0] == 0x40);
        for (int k = 1; k < 64; ++k) CHECK(b[k] == 0);
        return 0;
    }
    CHECK((b[0] >> 6) >= 2);
    ++n_flag[(b[0] >> 6) & 1];
    H::G2 back;
    const int32_t rc = H::g2_decompress_be(b, back);
    if (is_generator) { CHECK(rc == KZG_ERR_NOT_ON_CURVE); return 0; }
    CHECK(rc == KZG_OK);
    uint64_t w2[16];
    H::g2_to_wire(back, w2);
    CHECK(memcmp(w2, wire, 128) == 0);
    return 0;
}

int main() {
    std::vector<uint64_t> c(8), c2(16), pi2(16), zero(16, 0);
    const uint64_t lens[3] = {1, 4, 1024};
    // random-looking multiples; the search below extends the range until coordinates with a zero top byte have occurred
    for (uint64_t i = 0; i < 400 && (i < 40 || n_leading_zero < 3); ++i) {
        const uint64_t k[4] = {0x9E3779B97F4A7C15ULL * (i + 1), i, 7 * i + 1, 0}, k2[4] = {i + 1, 0xD1B54A32D192ED03ULL * (i + 3), 0, 0}, k3[4] = {3 * i + 2, i, 0, 0};
        H::g1_to_wire(H::g1_mul_generator(k), c.data());
        H::g2_to_wire(H::g2_mul_generator(k2), c2.data());
        H::g2_to_wire(H::g2_mul_generator(k3), pi2.data());
        if (check_header(lens[i % 3], c.data(), c2.data(), pi2.data())) return 1;
        if (check_encoder(c2.data(), false) || check_encoder(pi2.data(), false)) return 1;
        if (i < 8) {                                                   // the same x with the other y: the other sign flag of every element
            H::g1_to_wire(H::g1_neg(H::g1_mul_generator(k)), c.data());
            H::g2_to_wire(H::g2_neg(H::g2_mul_generator(k2)), c2.data());
            if (check_header(((uint64_t)1 << 40) + i, c.data(), c2.data(), pi2.data())) return 1;
            if (check_encoder(c2.data(), false)) return 1;
        }
    }
    CHECK(n_leading_zero >= 3);
    CHECK(n_flag[0] >= 8 && n_flag[1] >= 8);
    // identities: each element alone, then all three
    for (int mask = 1; mask < 8; ++mask) {
        if (mask != 1 && mask != 2 && mask != 4 && mask != 7) continue;
        if (check_header(4, mask & 1 ? zero.data() : c.data(), mask & 2 ? zero.data() : c2.data(), mask & 4 ? zero.data() : pi2.data())) return 1;
    }
    if (check_encoder(zero.data(), false)) return 1;
    {
        const uint64_t one[4] = {1, 0, 0, 0};
        H::g2_to_wire(H::g2_mul_generator(one), c2.data());
        if (check_encoder(c2.data(), true)) return 1;
        if (check_header(1, c.data(), c2.data(), c2.data())) return 1;
    }
    // a coordinate not below p: refused, each of the four
    for (int q = 0; q < 4; ++q) {
        std::vector<uint64_t> w(pi2);
        memcpy(w.data() + 4 * q, H::FQ_P.l, 32);
        uint8_t b[64];
        CHECK(!H::g2_encode_be(w.data(), b));
    }
    printf("headerbytescheck ok %d %d\n", n_headers, n_leading_zero);
    return 0;
}
