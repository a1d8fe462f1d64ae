// g2_decode.h — gnark-compressed G2 points -> affine points on the twist, per lane, on the Fq / Fq2 arithmetic of field29.h and fq2.h:
// the byte decode, the square root in Fq (one exponentiation by (p + 1) / 4, p = 3 mod 4), the square root in Fq2 by the norm method
// with TWO such exponentiations, the sign rule, and the decoder around them.  The format is that of the reference's
// `g2.point.powerOf2` (host_g2_decode.h): 64 bytes per point, X.A1 || X.A0 big-endian, the top two bits of the first byte 0b10 = the
// smaller y, 0b11 = the larger.
//
// Square root of a = a0 + a1 u, u^2 = -1.  a is a square in Fq2 exactly when its norm n = a0^2 + a1^2 is one
// in Fq.  With alpha = sqrt(n), delta = (a0 + alpha) / 2 and delta' = (a0 - alpha) / 2:  delta delta' = -a1^2 / 4, and -1 is not a
// square, so for a1 != 0 exactly one of delta, delta' is.  x0 = delta^((p + 1) / 4) squares to delta (then the root is
// (x0, a1 / (2 x0))) or to -delta (then a1 / (2 x0) squares to delta' and the root is (a1 / (2 x0), x0): the components trade places).
// No third exponentiation, and both outcomes are one select.  For a1 = 0 the second exponentiation takes a0 itself: its result squares
// to a0 (root (x0, 0)) or to -a0 (root (0, x0)), the same select with a1 / (2 x0) = 0.
//
// Every function is KZG_HD: hipcc compiles it for k_g2_decompress (g2decode.hip), g++ with -DKZG_BOUND_CHECK for
// tests/hostcheck/g2sqrtcheck.cpp, which compares every one BY VALUE with host_pairing.h / host_g2_decode.h.  Bounds are annotated per
// line as in fq2.h (class F: (-m, 2m); class O: (-0.0001m, 1.0001m); products as their value in m^2 against 169).
#pragma once
#include <cstddef>
#include "g2_chain.h"

namespace kzg {

// what a point fails, in the order of the checks (host_g2_decode.h g2_decompress_be); the device reports index << 2 | kind
constexpr uint32_t G2_BAD_DESERIALIZE = 0;      // flag bits not 0b10 / 0b11, or a coordinate not below the modulus
constexpr uint32_t G2_BAD_NO_POINT = 1;         // x^3 + b is not a square: no point of that x on the twist
constexpr uint32_t G2_BAD_SUBGROUP = 2;         // not in the order-r subgroup
constexpr uint32_t G2_BAD_GENERATOR = 3;        // the generator itself
constexpr uint32_t G2_DECODE_OK = 4;

// ---------------------------------------------------------------------------------------------
// bytes
// ---------------------------------------------------------------------------------------------
// 64 bytes -> the 16 words a little-endian load of them leaves (what the kernel reads as four uint4)
KZG_HD void g2_bytes_to_words(uint32_t raw[16], const uint8_t b[64]) {
    for (int j = 0; j < 16; ++j) raw[j] = (uint32_t)b[4 * j] | (uint32_t)b[4 * j + 1] << 8 | (uint32_t)b[4 * j + 2] << 16 | (uint32_t)b[4 * j + 3] << 24;
}
// 32 big-endian bytes (as 8 such words) -> internal form, class F; the return value: the integer, after top_mask on its highest word,
// is below the modulus.  The word order and the compare of k_srs_decompress (srs.hip), the compare without a branch.
KZG_HD bool fq_decode_be(Fq& r, const uint32_t raw[8], uint32_t top_mask) {
    uint32_t w32[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w32[k] = __builtin_bswap32(raw[7 - k]);      // little-endian word k = big-endian bytes 28 - 4k .. 31 - 4k
    w32[7] &= top_mask;
    bool below = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) below = w32[k] < FqParams::P32[k] ? true : (w32[k] > FqParams::P32[k] ? false : below);
    Fq t, kin;
    fe_unpack(t, w32);                             // [0, 2^256): below 5.3m
#pragma unroll
    for (int j = 0; j < NL; ++j) kin.l[j] = (int32_t)FqParams::K_PLAIN_IN[j];
    fe_mul(r, t, kin);                             // 5.3 * 1: class F
    return below;
}
// one compressed point -> its flag bits (0 .. 3) and x = (c0, c1) in class F; *below: both coordinates are below the modulus
KZG_HD uint32_t g2_decode_x_be(Fq2& x, bool& below, const uint32_t raw[16]) {
    const uint32_t flag = (raw[0] >> 6) & 3u;      // the top two bits of byte 0
    const bool b1 = fq_decode_be(x.c1, raw, 0x3FFFFFFFu);                    // X.A1 first, the flag bits masked out
    const bool b0 = fq_decode_be(x.c0, raw + 8, 0xFFFFFFFFu);
    below = b0 && b1;
    return flag;
}

// ---------------------------------------------------------------------------------------------
// square roots
// ---------------------------------------------------------------------------------------------
// 1 / 2 in the internal form (2^260 mod p), canonical
KZG_HD void fq_set_half(Fq& r) {
    const int32_t c[NL] = {0x16fce4b4, 0x0a904407, 0x0a626a11, 0x12109375, 0x1014a498, 0x100ec0c7, 0x093e16a4, 0x09c376ee, 0x001f1642};
#pragma unroll
    for (int j = 0; j < NL; ++j) r.l[j] = c[j];
}

// r = a^((p + 1) / 4) for a in class F, and whether r^2 == a (then r is a square root of a; otherwise r^2 == -a and a has none).
// The exponent is a constant of 252 bits = 84 digits of 3 bits, the top one 6: a table of a^1 .. a^7 (6 products), then per digit three
// squarings and at most one product: 249 squarings and <= 83 products instead of the ~126 of a bit-by-bit loop.  The digits are the
// same for every lane, so the table entry is chosen by selects on a uniform value and the loop stays rolled (one body in the kernel).
// Result in class F.
constexpr int G2_SQRT_WINDOW = 3, G2_SQRT_DIGITS = 84;
static_assert((FqParams::SQRT_EXP32[7] >> 28) == 0 && ((FqParams::SQRT_EXP32[7] >> 25) & 7u) == 6u, "(p + 1) / 4 has 252 bits, the top digit is 6");
KZG_HD bool fq_sqrt_candidate(Fq& r, const Fq& a) {
    Fq tbl[7];                                     // tbl[k] = a^(k + 1); every entry but the first a product: class F, any two 2 * 2 = 4
    tbl[0] = a;
    fe_sqr(tbl[1], a);                             // 2 * 2
    fe_mul(tbl[2], tbl[1], a);
    fe_sqr(tbl[3], tbl[1]);
    fe_mul(tbl[4], tbl[3], a);
    fe_sqr(tbl[5], tbl[2]);
    fe_mul(tbl[6], tbl[5], a);
    Fq acc = tbl[5];                               // the top digit
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = G2_SQRT_DIGITS - 2; i >= 0; --i) {
        fe_sqr(acc, acc); fe_sqr(acc, acc); fe_sqr(acc, acc);               // 2 * 2 each
        const int pos = G2_SQRT_WINDOW * i, wd = pos >> 5;
        const uint32_t hi = wd < 7 ? FqParams::SQRT_EXP32[wd + 1] : 0u;      // (a digit may straddle two words)
        const uint32_t d = (uint32_t)(((uint64_t)hi << 32 | FqParams::SQRT_EXP32[wd]) >> (pos & 31)) & 7u;
        if (d) {
            Fq m = tbl[0];
#pragma unroll
            for (int k = 1; k < 7; ++k) fe_select(m, d == (uint32_t)k + 1, tbl[k], m);
            fe_mul(acc, acc, m);                   // 2 * 2
        }
    }
    Fq t;
    fe_sqr(t, acc);
    fe_sub(t, t, a);                               // class F - class F: (-3m, 3m)
    fe_reduce_small(t);                            // class O
    r = acc;
    return fe_is_zero_mod(t);
}

// r = a square root of a (class F), or false when a is not a square; two exponentiations (the identity is at the top of the file).
// r in class F.
KZG_HD bool fq2_sqrt(Fq2& r, const Fq2& a) {
    Fq n0, n1, n, alpha, s, half, delta, din, x0, d, di, t;
    fe_sqr2(n0, a.c0, n1, a.c1);                   // 2 * 2 each
    fe_add(n, n0, n1);                             // (-2m, 4m)
    fe_reduce_small(n);                            // class O
    const bool square = fq_sqrt_candidate(alpha, n);                         // alpha^2 == n, or a is not a square
    fe_add(s, a.c0, alpha); fe_norm(s);            // (-2m, 4m)
    fq_set_half(half);
    fe_mul(delta, s, half);                        // 4 * 1: class F
    const bool a1_zero = fe_is_zero_mod(a.c1);
    fe_select(din, a1_zero, a.c0, delta);          // a1 == 0: a0 itself (delta is a0 or 0 there)
    const bool direct = fq_sqrt_candidate(x0, din);                          // x0^2 == din, else x0^2 == -din
    fe_dbl(d, x0);                                 // (-2m, 4m), limbs below 2^30
    fe_reduce_small(d);                            // class O, for the inversion's fe_canon
    fe_inverse_safegcd(di, d);                     // 1 / (2 x0), class F; 0 -> 0 (only for a1 == 0)
    fe_mul(t, a.c1, di);                           // 2 * 2: a1 / (2 x0), class F
    fe_select(r.c0, direct, x0, t);
    fe_select(r.c1, direct, t, x0);
    return square;
}

// ---------------------------------------------------------------------------------------------
// sign rule
// ---------------------------------------------------------------------------------------------
// the canonical integer of a (class F) is above (p - 1) / 2; *zero: it is 0
KZG_HD bool fq_plain_is_large(const Fq& a, bool& zero) {
    Fq one_plain, c;
    fe_set_zero(one_plain);
    one_plain.l[0] = 1;
    fe_mul(c, a, one_plain);                       // internal -> plain integer, class F
    fe_canon(c);
    uint32_t w[8];
    fe_pack(w, c);
    bool ge = true;                                // c >= (p + 1) / 2
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        ge = w[k] > FqParams::HALF_UP32[k] ? true : (w[k] < FqParams::HALF_UP32[k] ? false : ge);
        any |= w[k];
    }
    zero = any == 0;
    return ge;
}
// gnark's LexicographicallyLargest on (y.c1, y.c0): y.c1 > (p - 1) / 2, or y.c1 == 0 and y.c0 > (p - 1) / 2.  y in class F.
KZG_HD bool fq2_lexicographically_largest(const Fq2& y) {
    bool z0, z1;
    const bool l0 = fq_plain_is_large(y.c0, z0), l1 = fq_plain_is_large(y.c1, z1);
    return z1 ? l0 : l1;
}

// ---------------------------------------------------------------------------------------------
// one point
// ---------------------------------------------------------------------------------------------
// 64 bytes (as 16 words) -> the affine point on the twist, coordinates canonical like every G2Affine.  G2_DECODE_OK, or the first of
// G2_BAD_DESERIALIZE / G2_BAD_NO_POINT that applies; the subgroup and the generator are the caller's (g2_in_subgroup, g2_is_generator).
KZG_HD uint32_t g2_decompress_point(G2Affine& p, const uint32_t raw[16]) {
    Fq2 x, b, xx, y2, y;
    bool below;
    const uint32_t flag = g2_decode_x_be(x, below, raw);
    if (flag < 2 || !below) return G2_BAD_DESERIALIZE;
    g2_twist_b(b);
    fq2_sqr(xx, x);                                // 4 * 4
    fq2_mul_lazy(y2, xx, x);                       // 4 * 4: c0 in (-3m, 3m), c1 in (-5m, 4m)
    fq2_add(y2, y2, b);                            // + class F: c0 in (-4m, 5m), c1 in (-6m, 6m); limbs within +-(2^30 + 2^29)
    fq2_reduce(y2);                                // class O
    if (!fq2_sqrt(y, y2)) return G2_BAD_NO_POINT;
    const bool large = fq2_lexicographically_largest(y);
    fe_canon(y.c0); fe_canon(y.c1);                // [0, m) before the sign flip so that -y stays inside (-m, 2m)
    fq2_cneg(y, y, (flag == 3u) != large ? 1u : 0u);
    fq2_norm(y);                                   // (-m, m)
    fe_canon(x.c0); fe_canon(x.c1); fe_canon(y.c0); fe_canon(y.c1);
    p.x = x; p.y = y;
    return G2_DECODE_OK;
}
// p (canonical) is the generator of G2
KZG_HD bool g2_is_generator(const G2Affine& p) {
    uint32_t gw[32];
    g2_generator_wire(gw);
    Fq2 gx, gy;
    fq2_from_wire(gx, gw);
    fq2_from_wire(gy, gw + 16);
    fe_canon(gx.c0); fe_canon(gx.c1); fe_canon(gy.c0); fe_canon(gy.c1);
    uint32_t diff = 0;
#pragma unroll
    for (int j = 0; j < NL; ++j)
        diff |= (uint32_t)(p.x.c0.l[j] ^ gx.c0.l[j]) | (uint32_t)(p.x.c1.l[j] ^ gx.c1.l[j]) | (uint32_t)(p.y.c0.l[j] ^ gy.c0.l[j]) | (uint32_t)(p.y.c1.l[j] ^ gy.c1.l[j]);
    return diff == 0;
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------
// what the decode kernels share around g2_decompress_point (k_g2_decompress, k_header_g2_decode)
// ---------------------------------------------------------------------------------------------
// the 64 bytes of one point as four uint4
__device__ __forceinline__ void g2_load_raw(uint32_t raw[16], const uint4* __restrict__ src) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { const uint4 q = src[k]; raw[4 * k] = q.x; raw[4 * k + 1] = q.y; raw[4 * k + 2] = q.z; raw[4 * k + 3] = q.w; }
}
// a decoded point (canonical) as the 32 words it leaves in: wire words (WIRE) or the device format of curve_g2.h
template <bool WIRE>
__device__ __forceinline__ void g2_point_to_words(uint32_t o[32], const G2Affine& p) {
    if (WIRE) {
        fq2_to_wire(o, p.x);
        fq2_to_wire(o + 16, p.y);
    } else {
        fe_pack(o, p.x.c0); fe_pack(o + 8, p.x.c1); fe_pack(o + 16, p.y.c0); fe_pack(o + 24, p.y.c1);      // (canonical already)
    }
}
__device__ __forceinline__ void g2_store_words(uint4* __restrict__ dst, const uint32_t o[32]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
}
#endif

}  // namespace kzg
