// host_g2_decode.h — gnark-compressed G2 points -> wire form, on the host (kzg_g2_decompress_be, capi_g2.hip).  The format of the
// reference's `g2.point.powerOf2`: 64 bytes per point, X.A1 || X.A0 big-endian, the top two bits of the first byte 0b10 = the smaller
// y, 0b11 = the larger; "larger" compares (y.c1, y.c0) with (p - 1) / 2 as gnark's `LexicographicallyLargest` does.  The square root
// in Fq2 is the norm method on the host Fq of host_pairing.h (p = 3 mod 4: a^((p + 1) / 4)).  Pure host code; also compiled with g++
// under sanitizers by tests/hostcheck/g2_sanitize_main.cpp.
#pragma once
#include "../../include/kzg_bn254_mi355x.h"
#include "host_pairing.h"

namespace kzg_host {

inline Fq fq_from_plain(const Fq& a) { return mul(a, fq_r2()); }                               // integer a < p -> a R
inline Fq fq_to_plain(const Fq& a) { const Fq one = {{1, 0, 0, 0}}; return mul(a, one); }     // a R -> integer a
inline Fq fq_pow(const Fq& a, const Fq& e) {
    Fq acc = FQ_ONE;
    for (int i = 255; i >= 0; --i) {
        acc = sqr(acc);
        if ((e.l[i >> 6] >> (i & 63)) & 1) acc = mul(acc, a);
    }
    return acc;
}
// a square root of a, or false
inline bool fq_sqrt(const Fq& a, Fq& r) {
    static const Fq e = []() { Fq v = FQ_P; v.l[0] += 1; shr1(v); shr1(v); return v; }();       // (p + 1) / 4 (p = ..47 hex: no carry out of the low word)
    r = fq_pow(a, e);
    return eq(sqr(r), a);
}
// a square root of a0 + a1 u in Fq[u] / (u^2 + 1), or false
inline bool fq2_sqrt(const Fq2& a, Fq2& r) {
    if (is_zero(a.c1)) {
        Fq t;
        if (fq_sqrt(a.c0, t)) { r = {t, fq_zero()}; return true; }
        if (fq_sqrt(neg(a.c0), t)) { r = {fq_zero(), t}; return true; }
        return false;
    }
    Fq alpha;
    if (!fq_sqrt(add(sqr(a.c0), sqr(a.c1)), alpha)) return false;
    Fq s = add(a.c0, alpha), x0;
    half_mod_p(s);                                      // (halving commutes with the Montgomery radix)
    if (!fq_sqrt(s, x0)) {
        s = sub(a.c0, alpha);
        half_mod_p(s);
        if (!fq_sqrt(s, x0)) return false;
    }
    if (is_zero(x0)) return false;
    r = {x0, mul(a.c1, inv(dbl(x0)))};
    return true;
}
// y.c1 > (p - 1) / 2, or y.c1 == 0 and y.c0 > (p - 1) / 2, on the canonical integers
inline bool fq2_lexicographically_largest(const Fq2& y) {
    static const Fq half = []() { Fq v = FQ_P; shr1(v); return v; }();                          // (p - 1) / 2
    const Fq c1 = fq_to_plain(y.c1), c0 = fq_to_plain(y.c0);
    const Fq& v = is_zero(c1) ? c0 : c1;
    return geq(v, half) && !eq(v, half);
}
inline bool fq_from_be(const uint8_t b[32], uint8_t first_mask, Fq& out) {                      // false: not below the modulus
    Fq v;
    for (int j = 0; j < 4; ++j) {
        uint64_t w = 0;
        for (int k = 0; k < 8; ++k) { uint8_t byte = b[8 * (3 - j) + k]; if (j == 3 && k == 0) byte &= first_mask; w = (w << 8) | byte; }
        v.l[j] = w;
    }
    if (geq_p(v)) return false;
    out = fq_from_plain(v);
    return true;
}
// One point.  KZG_OK, or the status of the first check that fails, in the order of the Python decoder it replaces:
//   flag bits not 0b10 / 0b11 -> KZG_ERR_DESERIALIZE; a coordinate of x not below the modulus -> KZG_ERR_DESERIALIZE; x^3 + b not a square
//   (no such point on the twist) -> KZG_ERR_NOT_ON_CURVE; the point not in the order-r subgroup, or the generator itself
//   (example_validate_g2_point) -> KZG_ERR_NOT_ON_CURVE
inline int32_t g2_decompress_be(const uint8_t ch[64], G2& out) {
    const int flag = ch[0] >> 6;
    if (flag != 2 && flag != 3) return KZG_ERR_DESERIALIZE;
    Fq2 x;
    if (!fq_from_be(ch + 32, 0xFF, x.c0) || !fq_from_be(ch, 0x3F, x.c1)) return KZG_ERR_DESERIALIZE;
    const Fq2 b = {TWIST_B0, TWIST_B1};
    Fq2 y;
    if (!fq2_sqrt(add(mul(sqr(x), x), b), y)) return KZG_ERR_NOT_ON_CURVE;
    const bool large = fq2_lexicographically_largest(y);
    if ((flag == 3) != large) y = neg(y);
    out.x = x; out.y = y; out.inf = false;
    if (!g2_mul(out, FR_MODULUS_WORDS).inf) return KZG_ERR_NOT_ON_CURVE;
    const G2 g = g2_generator();
    if (eq(out.x, g.x) && eq(out.y, g.y)) return KZG_ERR_NOT_ON_CURVE;
    return KZG_OK;
}

}  // namespace kzg_host
