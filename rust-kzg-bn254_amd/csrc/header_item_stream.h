// header_item_stream.h — the message of one item digest of the header transcript (host_fiat_shamir.h header_batch_weights_host), produced
// block by block for a lane that hashes it with dev_sha256.h (k_header_item_digests of headerbytes.hip):
//
//     "KZGBN254_HEADERITEM__V1_" || u64be(d) || ark-compressed C || g2bytes(C2) || g2bytes(pi2)                      320 bytes
//
// 80 big-endian words, so the blocks fall on the parts: block 0 = tag (6 words), d (2), C (8); blocks 1, 2 = C2 (x then y, 16 words
// each); blocks 3, 4 = pi2; block 5 = the pad byte and the bit length.  No block carries anything into the next.
//   C    comes from its SERIALIZED form as it arrived (g1_decode.h: 32 gnark-compressed bytes, as the words a little-endian load leaves):
//        the bytes reversed with the flag bits remapped (0b10 -> 0, 0b11 -> 0x80, 0b01 -> 0x40, 0b00 -> 0xC0), as CosetItemBytesSrc of
//        coset_item_stream.h does; no field arithmetic.
//   C2, pi2 come from the DECODED point in the device format of curve_g2.h (x.c0 | x.c1 | y.c0 | y.c1, each the packed canonical residue
//        of the internal form a 2^261): one product by the plain 1 per coordinate gives the integer a, written big-endian.  The identity
//        is 32 zero words in and 128 zero bytes out.
// For every header that decodes these are the bytes the host transcript hashes from the wire points.  Every function is KZG_HD: hipcc
// compiles it for the kernel, g++ for tests/hostcheck/headerbytescheck.cpp.
#pragma once
#include "coset_item_stream.h"

namespace kzg {

constexpr uint32_t HEADER_ITEM_LEN = 320, HEADER_ITEM_BLOCKS = 6;
static_assert(HEADER_ITEM_LEN == 24 + 8 + 32 + 128 + 128 && HEADER_ITEM_LEN % 64 == 0, "five whole blocks of message, one of padding");

struct HeaderItemSrc {
    const uint32_t* commitment_be;   // 8 words of gnark-compressed bytes (16-byte aligned)
    const uint32_t* c2;              // 32 words, device affine format (16-byte aligned)
    const uint32_t* pi2;             // the same
    uint64_t d;                      // the claimed length
};

// one coordinate: the packed internal form -> the 8 big-endian words of be32(a)
KZG_HD void header_item_coord(uint32_t out[8], const uint32_t* p) {
    uint32_t w[8], c[8];
    coset_item_load8(w, p);
    Fq t, one_plain;
    fe_unpack(t, w);                               // canonical: [0, m)
    fe_set_zero(one_plain);
    one_plain.l[0] = 1;
    fe_mul(t, t, one_plain);                       // a 2^261 * 2^-261 = a, class F
    fe_canon(t);
    fe_pack(c, t);
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = c[7 - j];
}

// the 16 words of block b < HEADER_ITEM_BLOCKS, padding and length included
KZG_HD void header_item_block(uint32_t w[16], const HeaderItemSrc& s, uint32_t b) {
    if (b == 0) {
        w[0] = 0x4b5a4742u; w[1] = 0x4e323534u; w[2] = 0x5f484541u; w[3] = 0x44455249u; w[4] = 0x54454d5fu; w[5] = 0x5f56315fu;   // the tag
        w[6] = (uint32_t)(s.d >> 32); w[7] = (uint32_t)s.d;
        uint32_t g[8];
        coset_item_load8(g, s.commitment_be);
#pragma unroll
        for (int j = 0; j < 8; ++j) w[8 + j] = g[7 - j];                // the reversed bytes as big-endian words: the loaded words in reverse order, unswapped
        const uint32_t f = (g[0] >> 6) & 3u;                            // the top two bits of gnark's byte 0 = ark's byte 31 = the low byte of w[15]
        const uint32_t flag = f == 0u ? 0xC0u : f == 1u ? 0x40u : f == 2u ? 0u : 0x80u;
        w[15] = (w[15] & ~0xC0u) | flag;
    } else if (b < HEADER_ITEM_BLOCKS - 1) {
        const uint32_t* p = (b <= 2 ? s.c2 : s.pi2) + 16 * ((b - 1) & 1u);     // x on the odd blocks, y on the even ones
        header_item_coord(w, p);
        header_item_coord(w + 8, p + 8);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = 0;
        w[0] = 0x80000000u;
        w[15] = HEADER_ITEM_LEN * 8;
    }
}

// the whole digest of one header, as the 8 words sha256_digest_le_words leaves (a little-endian store of them is the 32 digest bytes)
KZG_HD void header_item_digest(uint32_t out[8], const HeaderItemSrc& s) {
    uint32_t st[8], w[16];
    sha256_init_state(st);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint32_t b = 0; b < HEADER_ITEM_BLOCKS; ++b) {
        header_item_block(w, s, b);
        sha256_compress(st, w);
    }
    sha256_digest_le_words(out, st);
}

}  // namespace kzg
