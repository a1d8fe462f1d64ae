// g1_decode.h — one gnark-compressed G1 point -> its affine coordinates, per lane, STRICT: the decoder of the points a verifier gets off
// the wire (cosetbytes.hip).  32 big-endian bytes, the top two bits of byte 0: 0b00 = gnark's uncompressed marker (a 32-byte point
// cannot carry it), 0b01 = the identity (every other bit zero), 0b10 / 0b11 = the smaller / larger y.  The checks, in this order:
//
//   1. flags                                                    G1_BAD_DESERIALIZE
//   2. x canonical: x >= p is refused (NOT reduced)             G1_BAD_DESERIALIZE
//   3. y = (x^3 + 3)^((p + 1) / 4), y^2 == x^3 + 3              G1_BAD_NOT_ON_CURVE
//   4. the sign by lexicographically_largest (y > (p - 1) / 2 on the canonical integer)
//
// Rule 2 is stricter than the SRS loader (k_srs_decompress of srs.hip reduces x mod p, as the reference's from_be_bytes_mod_order
// does): here one byte string names one point, so that a transcript over the bytes equals the transcript over the decoded points.
// The exponentiation is the fixed 3-bit window of g2_decode.h (fq_sqrt_candidate: 249 squarings, at most 89 products), the byte
// decode and the sign rule are that header's too.  G1 has cofactor 1: a point on the curve is in the group.
//
// The way out is here too: g1_compress_point, the inverse of g1_decompress_point, which the affine conversion behind FK20 ends in when the
// encoder writes bytes (g1fft.hip k_g1fft_to_affine<true>), and the scalar codec both ways (recover.hip, multiproof.hip).
//
// Every function is KZG_HD: hipcc compiles it for the kernels of cosetbytes.hip, recover.hip, multiproof.hip and g1fft.hip, g++ with -DKZG_BOUND_CHECK for
// tests/hostcheck/g1decodecheck.cpp and tests/hostcheck/g1compresscheck.cpp.  Bounds per line as in g2_decode.h (class F: (-m, 2m); class O: (-0.0001m, 1.0001m)).
#pragma once
#include "g2_decode.h"

namespace kzg {

// what a point fails, in the order of the checks; the device reports index << 2 | kind
constexpr uint32_t G1_BAD_DESERIALIZE = 0;      // flag bits 0b00, a marked identity with other bits set, or x not below the modulus
constexpr uint32_t G1_BAD_NOT_ON_CURVE = 1;     // x^3 + 3 is not a square: no point of that x on the curve
constexpr uint32_t G1_DECODE_OK = 4;            // a finite point
constexpr uint32_t G1_DECODE_IDENTITY = 5;      // the identity (x and y are set to zero)

// 32 bytes -> the 8 words a little-endian load of them leaves (what the kernel reads as two uint4)
KZG_HD void g1_bytes_to_words(uint32_t raw[8], const uint8_t b[32]) {
    for (int j = 0; j < 8; ++j) raw[j] = (uint32_t)b[4 * j] | (uint32_t)b[4 * j + 1] << 8 | (uint32_t)b[4 * j + 2] << 16 | (uint32_t)b[4 * j + 3] << 24;
}

// 32 bytes (as 8 words) -> x and y in the internal form, canonical [0, m).  G1_DECODE_OK / G1_DECODE_IDENTITY, or the first of
// G1_BAD_DESERIALIZE / G1_BAD_NOT_ON_CURVE that applies (x and y are then unspecified).
KZG_HD uint32_t g1_decompress_point(Fq& x, Fq& y, const uint32_t raw[8]) {
    const uint32_t flag = (raw[0] >> 6) & 3u;      // the top two bits of byte 0
    if (flag == 0u) return G1_BAD_DESERIALIZE;
    if (flag == 1u) {
        uint32_t rest = raw[0] & ~0xC0u;
#pragma unroll
        for (int k = 1; k < 8; ++k) rest |= raw[k];
        fe_set_zero(x);
        fe_set_zero(y);
        return rest ? G1_BAD_DESERIALIZE : G1_DECODE_IDENTITY;
    }
    if (!fq_decode_be(x, raw, 0x3FFFFFFFu)) return G1_BAD_DESERIALIZE;       // x in class F
    Fq t, y2, b3;
#pragma unroll
    for (int j = 0; j < NL; ++j) b3.l[j] = (int32_t)FqParams::B3[j];
    fe_sqr(t, x);                                  // 2 * 2
    fe_mul(y2, t, x);                              // 2 * 2
    fe_add(y2, y2, b3);                            // class F + [0, m): (-m, 3m)
    fe_reduce_small(y2);                           // class O
    if (!fq_sqrt_candidate(y, y2)) return G1_BAD_NOT_ON_CURVE;               // y in class F, y^2 == x^3 + 3
    bool zero;
    const bool large = fq_plain_is_large(y, zero);                           // (y == 0 would need x^3 == -3: -3 is no cube in Fq, the curve has odd order)
    fe_canon(y);                                   // [0, m) before the sign flip so that -y stays inside (-m, 2m)
    fe_cneg(y, y, (flag == 3u) != large ? 1u : 0u);
    fe_norm(y);                                    // (-m, m)
    fe_canon(x);
    fe_canon(y);
    return G1_DECODE_OK;
}

// The way out, the inverse of g1_decompress_point: an affine point in the internal form (x, y in class F; ignored for the identity) -> the
// 32 gnark bytes as the 8 words a little-endian store of them takes.  x leaves canonical and big-endian, the flag is 0b10 / 0b11 by the
// decoder's own rule (fq_plain_is_large on the canonical y), the identity is 0x40 followed by zeros: kzg_host::g1_encode_be (host_coset_bytes.h)
// byte for byte.
KZG_HD void g1_compress_point(uint32_t raw[8], const Fq& x, const Fq& y, bool identity) {
    if (identity) {
        raw[0] = 0x40u;                            // byte 0
#pragma unroll
        for (int k = 1; k < 8; ++k) raw[k] = 0u;
        return;
    }
    Fq one_plain, c;
    fe_set_zero(one_plain);
    one_plain.l[0] = 1;
    fe_mul(c, x, one_plain);                       // 2 * 1: internal -> plain integer, class F
    fe_canon(c);                                   // [0, m)
    uint32_t w32[8];
    fe_pack(w32, c);
#pragma unroll
    for (int k = 0; k < 8; ++k) raw[k] = __builtin_bswap32(w32[7 - k]);      // big-endian bytes 4k .. 4k + 3 = little-endian word 7 - k
    bool zero;
    const bool large = fq_plain_is_large(y, zero);                           // y in class F
    raw[0] |= large ? 0xC0u : 0x80u;               // x < p < 2^254 leaves the top two bits of byte 0 free
}
// the same from a wire point (arkworks Montgomery words, canonical; the all-zero point is the identity, as the wire outputs write it)
KZG_HD void g1_compress_wire_point(uint32_t raw[8], const uint32_t wire[16]) {
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) any |= wire[k];
    Fq x, y;
    fe_from_wire(x, wire);                         // 5.3 * 1: class F
    fe_from_wire(y, wire + 8);
    g1_compress_point(raw, x, y, any == 0);
}

// the point in the device format of curve.h (x || y, canonical internal limbs packed to 2 x 8 words); the identity is 16 zero words, which
// is what the upload path writes for the all-zero wire point
KZG_HD void g1_point_to_device_words(uint32_t o[16], const Fq& x, const Fq& y) {
    fe_pack(o, x);
    fe_pack(o + 8, y);
}
// ... and as a wire point (arkworks Montgomery words); the identity is 16 zero words, its flag travels beside it
KZG_HD void g1_point_to_wire_words(uint32_t o[16], const Fq& x, const Fq& y) {
    fe_to_wire(o, x);
    fe_to_wire(o + 8, y);
}

// 32 big-endian bytes of a scalar (as 8 words) -> wire form (arkworks Montgomery words, canonical); false: the integer is not below r
KZG_HD bool fr_decode_be_to_wire(uint32_t out[8], const uint32_t raw[8]) {
    uint32_t w32[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w32[k] = __builtin_bswap32(raw[7 - k]);      // little-endian word k = big-endian bytes 28 - 4k .. 31 - 4k
    bool below = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) below = w32[k] < FrParams::P32[k] ? true : (w32[k] > FrParams::P32[k] ? false : below);
    Fr t, kin;
    fe_unpack(t, w32);                             // [0, 2^256): below 5.3m
#pragma unroll
    for (int j = 0; j < NL; ++j) kin.l[j] = (int32_t)FrParams::K_RAW[j];
    fe_mul(t, t, kin);                             // 5.3 * 1: v 2^256 in (-m, 2m)
    fe_canon(t);
    fe_pack(out, t);
    return below;
}
// the way back: wire form (canonical) -> the 32 big-endian bytes of the integer (as 8 words), the exact inverse of fr_decode_be_to_wire
// on every canonical wire element
KZG_HD void fr_encode_wire_to_be(uint32_t out_raw[8], const uint32_t wire[8]) {
    uint32_t w32[8];
    fe_wire_to_canonical_words<FrParams>(w32, wire);                         // [0, 2^256) below 5.3m, times 32: the integer in [0, m)
#pragma unroll
    for (int k = 0; k < 8; ++k) out_raw[k] = __builtin_bswap32(w32[7 - k]);
}

}  // namespace kzg
