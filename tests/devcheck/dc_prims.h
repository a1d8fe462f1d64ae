// tests/devcheck/dc_prims.h -- TEST-ONLY: one field primitive of csrc/field29.h / fe_invert.h applied to raw limbs, the same code for
// the host build (tests/hostcheck/hostcheck.cpp, g++ with KZG_BOUND_CHECK) and the device builds (tests/devcheck/devcheck.hip, with
// and without the generated inline-asm products).  Operands: 4 x 9 int32 (a, b, c, d); results: 2 x 9 int32 (r, s).  Wire words
// travel in the first 8 limbs of a slot, reinterpreted as uint32.  The op numbers are mirrored in tests/fe_operands.py.
#pragma once
#include "field29.h"
#include "fe_invert.h"
#include "curve.h"
#include "naf.h"
#include <cstring>

namespace kzg {

enum DcOp {
    DC_MUL, DC_SQR, DC_MUL2, DC_SQR2, DC_MULSUB, DC_MUL_ILP,
    DC_ADD, DC_SUB, DC_DBL, DC_NORM, DC_CANON, DC_IS_ZERO_MOD, DC_REDUCE, DC_REDUCE_SMALL,
    DC_FROM_WIRE, DC_TO_WIRE, DC_WIRE_TO_CANONICAL, DC_INVERT,
    DC_OPS
};

template <class F>
KZG_HD void dc_apply(int op, const int32_t* in, int32_t* out) {
    Fe<F> a, b, c, d, r, s;
    for (int j = 0; j < NL; ++j) { a.l[j] = in[j]; b.l[j] = in[NL + j]; c.l[j] = in[2 * NL + j]; d.l[j] = in[3 * NL + j]; }
    fe_set_zero(r);
    fe_set_zero(s);
    uint32_t w[8], v[8];
    for (int j = 0; j < 8; ++j) w[j] = (uint32_t)in[j];
    switch (op) {
        case DC_MUL: fe_mul(r, a, b); break;
        case DC_SQR: fe_sqr(r, a); break;
        case DC_MUL2: fe_mul2(r, a, b, s, c, d); break;
        case DC_SQR2: fe_sqr2(r, a, s, c); break;
        case DC_MULSUB: fe_mulsub(r, a, b, c, d); break;
        case DC_MUL_ILP: fe_mul_ilp(r, a, b); break;
        case DC_ADD: fe_add(r, a, b); break;
        case DC_SUB: fe_sub(r, a, b); break;
        case DC_DBL: fe_dbl(r, a); break;
        case DC_NORM: r = a; fe_norm(r); break;
        case DC_CANON: r = a; fe_canon(r); break;
        case DC_IS_ZERO_MOD: r.l[0] = fe_is_zero_mod(a) ? 1 : 0; break;
        case DC_REDUCE: r = a; fe_reduce(r); break;
        case DC_REDUCE_SMALL: r = a; fe_reduce_small(r); break;
        case DC_FROM_WIRE: fe_from_wire(r, w); break;
        case DC_TO_WIRE: fe_to_wire(v, a); for (int j = 0; j < 8; ++j) r.l[j] = (int32_t)v[j]; break;
        case DC_WIRE_TO_CANONICAL: fe_wire_to_canonical_words<F>(v, w); for (int j = 0; j < 8; ++j) r.l[j] = (int32_t)v[j]; break;
        case DC_INVERT: fe_inverse_safegcd(r, a); break;
        default: break;
    }
    for (int j = 0; j < NL; ++j) { out[j] = r.l[j]; out[NL + j] = s.l[j]; }
}

// Point formulas of curve.h.  Input row: P1 and P2 as affine wire points (16 u32 each, zeros = identity) and a sign word; output: the
// XYZZ wire words (32 u32, X || Y || ZZ || ZZZ, zeros = identity).  P2 is never the identity (xyzz_madd's callers skip it).
//   DC_MADD: P1 + (sign ? -P2 : P2) by xyzz_madd        (P1 == +-P2 and P1 == identity reach the exceptional branches)
//   DC_PADD: (P1 + P2) + 2 P2 by xyzz_add               (P1 == P2: same point; P1 == -3 P2: opposite points; P1 == -P2: identity + Q)
//   DC_PDBL: 2 (P1 + P2) by xyzz_dbl                     (P1 == -P2: the identity doubled)
enum DcCurveOp { DC_MADD, DC_PADD, DC_PDBL, DC_CURVE_OPS };

KZG_HD bool dc_load_point(Affine& p, const uint32_t* wire) {
    uint32_t dev[16];
    affine_wire_to_device(dev, wire);
    uint4 v[4];
    memcpy(v, dev, sizeof(v));
    return affine_load(p, v);
}
KZG_HD void dc_curve(int op, const uint32_t* in, uint32_t* out) {
    Affine p1, p2;
    const bool has1 = dc_load_point(p1, in);
    dc_load_point(p2, in + 16);
    const uint32_t neg = in[32] & 1u;
    Xyzz a, r;
    if (has1) xyzz_from_affine(a, p1, 0); else xyzz_set_inf(a);
    if (op == DC_MADD) {
        xyzz_madd(a, p2, neg);
        r = a;
    } else if (op == DC_PADD) {
        xyzz_madd(a, p2, 0);
        Xyzz b, b2;
        xyzz_from_affine(b, p2, 0);
        xyzz_dbl(b2, b);
        xyzz_add(r, a, b2);
    } else {
        xyzz_madd(a, p2, 0);
        xyzz_dbl(r, a);
    }
    xyzz_to_wire(out, r);
}

// Width-w NAF recoding of naf.h.  Input: 8 u32 words of the scalar; output: out[0] = digit count, out[1 + t] =
// neg << 31 | pos << 20 | key for the first 63 digits.
KZG_HD void dc_naf(const uint32_t* in, int w, uint32_t* out) {
    uint32_t k[8];
    for (int j = 0; j < 8; ++j) k[j] = in[j];
    uint32_t n = 0;
    naf_for_digits(k, w, [&](uint32_t pos, uint32_t key, uint32_t neg) {
        if (n < 63) out[1 + n] = (neg << 31) | (pos << 20) | key;
        ++n;
    });
    out[0] = n;
}

}  // namespace kzg
