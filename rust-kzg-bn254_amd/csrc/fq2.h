// fq2.h — Fq2 = Fq[u] / (u^2 + 1) over the signed 9 x 29-bit Fq of field29.h: the coordinate field of BN254's G2 (curve_g2.h).
//
// An element is c0 + c1 u.  Ranges used below (all NORMALISED: limbs 0..7 in [0, 2^29), the top limb carries the sign):
//   class F   both components in (-m, 2m)                 any fe_mul / fe_sqr result; what fe_is_zero_mod and fe_canon accept
//   class O   both components in (-0.0001m, 1.0001m)      any fe_reduce_small result; O is inside F
// fq2_sqr leaves class F, fq2_mul leaves class O, fq2_mul_lazy leaves unreduced differences of products for the caller to combine.
//
// Where the signed bounds of fe_mul (|a b| < 2^261 m ~ 169 m^2, |a_j| |b_j| < 2^59.35) bind in this file:
//   Karatsuba multiplies the SUMS a0 + a1 and b0 + b1: their value is up to twice a component's, so a product of operands with
//   |a_i| < A m and |b_i| < B m needs 4 A B < 169, and their limbs are up to 2^30 before normalisation (2^60 per limb pair: over the
//   bound), so both sums are normalised first;
//   the results t0 - t1 in (-3m, 3m) and t2 - t0 - t1 in (-5m, 4m) are DIFFERENCES of products with limbs in (-2^30, 2^29): fed to
//   the next Karatsuba unreduced, 4 * 5 * 5 = 100 would still pass but a difference of two such values (every P = U2 - X1 of a group
//   law) would not, and their limb sums could leave int32.  So every product is reduced once, without a field product
//   (fe_reduce_small: ~70 instructions against the 206 of fe_mul), and the group law's bounds are those of curve.h or tighter.
// The KZG_BOUND_CHECK host build (tests/hostcheck/g2check.cpp) and the KZG_DEVICE_BOUND_CHECK build check every one of these.
//
// Replaces: ark-bn254's `Fq2` (QuadExtField over Fq with nonresidue -1) behind `G2Projective` in the protocol's length commitment
// and length proof.
#pragma once
#include "field29.h"
#include "fe_invert.h"

namespace kzg {

struct Fq2 {
    Fq c0, c1;
};

KZG_HD void fq2_set_zero(Fq2& r) { fe_set_zero(r.c0); fe_set_zero(r.c1); }
KZG_HD void fq2_set_one(Fq2& r) { fe_set_one(r.c0); fe_set_zero(r.c1); }
// lazy, limb-wise (no carry, no reduction): the bounds are the caller's
KZG_HD void fq2_add(Fq2& r, const Fq2& a, const Fq2& b) { fe_add(r.c0, a.c0, b.c0); fe_add(r.c1, a.c1, b.c1); }
KZG_HD void fq2_sub(Fq2& r, const Fq2& a, const Fq2& b) { fe_sub(r.c0, a.c0, b.c0); fe_sub(r.c1, a.c1, b.c1); }
KZG_HD void fq2_dbl(Fq2& r, const Fq2& a) { fe_dbl(r.c0, a.c0); fe_dbl(r.c1, a.c1); }
KZG_HD void fq2_neg(Fq2& r, const Fq2& a) { fe_neg(r.c0, a.c0); fe_neg(r.c1, a.c1); }
KZG_HD void fq2_cneg(Fq2& r, const Fq2& a, uint32_t neg) { fe_cneg(r.c0, a.c0, neg); fe_cneg(r.c1, a.c1, neg); }
KZG_HD void fq2_norm(Fq2& a) { fe_norm(a.c0); fe_norm(a.c1); }
// any lazy value with |c_i| < 169 m -> class O
KZG_HD void fq2_reduce(Fq2& a) { fe_reduce_small(a.c0); fe_reduce_small(a.c1); }
KZG_HD void fq2_select(Fq2& r, bool c, const Fq2& a, const Fq2& b) { fe_select(r.c0, c, a.c0, b.c0); fe_select(r.c1, c, a.c1, b.c1); }

// a in class F: a == 0 in Fq2
KZG_HD bool fq2_is_zero_mod(const Fq2& a) { const bool z0 = fe_is_zero_mod(a.c0), z1 = fe_is_zero_mod(a.c1); return z0 && z1; }
KZG_HD bool fq2_is_literal_zero(const Fq2& a) { const bool z0 = fe_is_literal_zero(a.c0), z1 = fe_is_literal_zero(a.c1); return z0 && z1; }

// Karatsuba, three fe_mul: t0 = a0 b0, t1 = a1 b1, t2 = (a0 + a1)(b0 + b1);  a b = (t0 - t1) + (t2 - t0 - t1) u.
// Operands: limbs within +-2^29 (normalised values or differences of two), (|a0| + |a1|)(|b0| + |b1|) < 169 m^2.
// Result UNREDUCED and not normalised: c0 in (-3m, 3m) with limbs in (-2^29, 2^29), c1 in (-5m, 4m) with limbs in (-2^30, 2^29).
KZG_HD void fq2_mul_lazy(Fq2& r, const Fq2& a, const Fq2& b) {
    Fq sa, sb, t0, t1, t2;
    fe_add(sa, a.c0, a.c1); fe_norm(sa);       // limbs up to 2^30 before: normalised for the limb bound of the product
    fe_add(sb, b.c0, b.c1); fe_norm(sb);
    fe_mul2(t0, a.c0, b.c0, t1, a.c1, b.c1);   // each in (-m, 2m)
    fe_mul(t2, sa, sb);
    fe_sub(r.c0, t0, t1);                      // (-3m, 3m)
    fe_sub(t2, t2, t0);
    fe_sub(r.c1, t2, t1);                      // (-5m, 4m)
}
// the same, reduced: class O
KZG_HD void fq2_mul(Fq2& r, const Fq2& a, const Fq2& b) {
    Fq2 t;
    fq2_mul_lazy(t, a, b);
    fq2_reduce(t);
    r = t;
}
// Two-product form: a^2 = (a0 + a1)(a0 - a1) + (2 a0) a1 u.  Operands: limbs within +-2^29, (|a0| + |a1|)^2 < 169 m^2 (|a_i| < 6.5m).
// Sum, difference and double have limbs up to 2^30: normalised first.  Both results are fe_mul outputs: class F, no reduction.
KZG_HD void fq2_sqr(Fq2& r, const Fq2& a) {
    Fq s, d, e, c0, c1;
    fe_add(s, a.c0, a.c1); fe_norm(s);
    fe_sub(d, a.c0, a.c1); fe_norm(d);
    fe_dbl(e, a.c0); fe_norm(e);
    fe_mul2(c0, s, d, c1, e, a.c1);
    r.c0 = c0; r.c1 = c1;
}
// a k for k in Fq (limbs within +-2^29, |a_i| |k| < 169 m^2): class F
KZG_HD void fq2_mul_fq(Fq2& r, const Fq2& a, const Fq& k) {
    Fq c0, c1;
    fe_mul2(c0, a.c0, k, c1, a.c1, k);
    r.c0 = c0; r.c1 = c1;
}
// 1 / a = (a0 - a1 u) / (a0^2 + a1^2), a in class F; 0 -> 0.  The norm is inverted by fe_invert.h's division steps.  Class F.
KZG_HD void fq2_inv(Fq2& r, const Fq2& a) {
    Fq n0, n1, n, ni, na1;
    fe_sqr2(n0, a.c0, n1, a.c1);               // 4 m^2 each
    fe_add(n, n0, n1);                         // (-2m, 4m)
    fe_reduce_small(n);                        // (-m, 2m) for the inversion's fe_canon
    fe_inverse_safegcd(ni, n);
    fe_neg(na1, a.c1); fe_norm(na1);           // (-2m, m)
    fe_mul2(r.c0, a.c0, ni, r.c1, na1, ni);
}

// ---------------------------------------------------------------------------------------------
// Wire format (arkworks Montgomery, radix 2^256, canonical): 16 u32 = c0[8] || c1[8]
// ---------------------------------------------------------------------------------------------
KZG_HD void fq2_from_wire(Fq2& r, const uint32_t w[16]) { fe_from_wire(r.c0, w); fe_from_wire(r.c1, w + 8); }     // class F
KZG_HD void fq2_to_wire(uint32_t w[16], const Fq2& a) { fe_to_wire(w, a.c0); fe_to_wire(w + 8, a.c1); }           // a normalised, |a_i| < 169 m
// class F -> canonical residues of the internal form, packed (the device-resident form of an affine coordinate)
KZG_HD void fq2_pack_canonical(uint32_t w[16], const Fq2& a) {
    Fq x = a.c0, y = a.c1;
    fe_canon(x); fe_canon(y);
    fe_pack(w, x); fe_pack(w + 8, y);
}
KZG_HD void fq2_unpack(Fq2& r, const uint32_t w[16]) { fe_unpack(r.c0, w); fe_unpack(r.c1, w + 8); }

}  // namespace kzg
