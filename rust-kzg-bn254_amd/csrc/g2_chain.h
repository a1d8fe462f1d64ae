// g2_chain.h — per-lane scalar chains on BN254's twist, on the Fq2 / XYZZ arithmetic of fq2.h and curve_g2.h: the twist Frobenius psi,
// [x]P for the BN parameter x, the order-r subgroup test built on them, and a double-and-add over a caller's scalar.  One lane (or one
// host call) per point; every lane of a launch runs the same trip counts.
//
// The inputs are ADVERSARIAL (G2 elements of a blob header come from an untrusted party): points of small order, P == +-Q and the
// identity do occur inside the chains, so every addition is one of the checked forms of curve_g2.h.
//
// Subgroup test: P is in the order-r subgroup of the twist iff
//     [x + 1]P + psi([x]P) + psi^2([x]P) == psi^3([2x]P)
// (gnark-crypto's G2Affine.IsInSubGroup for bn254; El Housni, Guillevic, Piellard, "Co-factor clearing and subgroup membership testing
// on pairing-friendly curves", 2022).  One 63-bit chain instead of the 254-bit [r]P.
//
// Compiled by hipcc for the kernels of g2batch.hip and by g++ with -DKZG_BOUND_CHECK for tests/hostcheck/g2chaincheck.cpp, which
// compares every function BY VALUE with host_pairing.h.
#pragma once
#include "curve_g2.h"

namespace kzg {

// gamma_x = xi^((p - 1) / 3), gamma_y = xi^((p - 1) / 2), xi = 9 + u: canonical residues of the internal Montgomery form (a 2^261 mod p)
// in 29-bit limbs.  The same values as TWIST_FROB_X0 .. TWIST_FROB_Y1 of pairing_constants.h (checked by g2cc_psi_constants).
KZG_HD void g2_psi_constants(Fq2& gx, Fq2& gy) {
    const int32_t c[4][NL] = {{0x04a59190, 0x06f504d9, 0x0bf870bb, 0x171ffd5c, 0x1ac4d17d, 0x04be36d5, 0x0bceec27, 0x1a83a513, 0x002492b3},
                              {0x11142ef1, 0x0b31acc7, 0x1d5818bc, 0x180afc17, 0x1a63177e, 0x15765b3b, 0x118f742e, 0x063a509a, 0x00135e4e},
                              {0x1b1f0678, 0x0373fb06, 0x13170fbd, 0x185d74b7, 0x0241131f, 0x16e18435, 0x1ef3b6ce, 0x01f06f02, 0x001d46bd},
                              {0x19a647d5, 0x19fdefab, 0x1d925d1a, 0x0d1f6c5f, 0x08ac6cc5, 0x1fa5621a, 0x134f06fe, 0x09a72816, 0x0015871d}};
#pragma unroll
    for (int j = 0; j < NL; ++j) { gx.c0.l[j] = c[0][j]; gx.c1.l[j] = c[1][j]; gy.c0.l[j] = c[2][j]; gy.c1.l[j] = c[3][j]; }
}

// conj(a) gamma for a in class F: the negated component is in (-2m, m), |.| < 2m: (2 + 2)(1 + 1) = 8 m^2.  Class O.
KZG_HD void fq2_conj_mul(Fq2& r, const Fq2& a, const Fq2& gamma) {
    Fq2 t;
    t.c0 = a.c0;
    fe_neg(t.c1, a.c1); fe_norm(t.c1);
    fq2_mul(r, t, gamma);
}
// conj(a) for a in class F, back in class O (the stored form wants (-m, 2m); -c1 alone is in (-2m, m))
KZG_HD void fq2_conj(Fq2& r, const Fq2& a) {
    r.c0 = a.c0;
    fe_neg(r.c1, a.c1);
    fe_reduce_small(r.c1);
}

// the twist Frobenius (x, y) -> (conj(x) gamma_x, conj(y) gamma_y); coordinates canonical on return, like every G2Affine
KZG_HD void g2_psi(G2Affine& p) {
    Fq2 gx, gy, x, y;
    g2_psi_constants(gx, gy);
    fq2_conj_mul(x, p.x, gx);
    fq2_conj_mul(y, p.y, gy);
    fe_canon(x.c0); fe_canon(x.c1); fe_canon(y.c0); fe_canon(y.c1);
    p.x = x; p.y = y;
}
// psi on a stored XYZZ value acts coordinate-wise: x = X / ZZ, y = Y / ZZZ, so X and Y take the constants and ZZ, ZZZ only the
// conjugation (ZZ^3 = ZZZ^2 is kept).  Stored form in, stored form out.
KZG_HD void g2_psi_xyzz(G2Xyzz& v) {
    if (v.inf) return;
    Fq2 gx, gy, t;
    g2_psi_constants(gx, gy);
    fq2_conj_mul(t, v.x, gx); v.x = t;
    fq2_conj_mul(t, v.y, gy); v.y = t;
    fq2_conj(t, v.zz); v.zz = t;
    fq2_conj(t, v.zzz); v.zzz = t;
}

// the BN parameter x = 0x44e992b44a6909f1 (BN_X of host_pairing.h), 63 bits, as two words
constexpr uint32_t G2_BN_X_LO = 0x4a6909f1u, G2_BN_X_HI = 0x44e992b4u;
constexpr int G2_BN_X_BITS = 63;

// out = [x]P, P affine and not the identity: 62 doublings and 27 mixed additions after the top bit, the same for every lane
KZG_HD void g2_mul_x(G2Xyzz& out, const G2Affine& p) {
    G2Xyzz acc;
    g2_from_affine(acc, p, 0);
#pragma unroll 1
    for (int bit = G2_BN_X_BITS - 2; bit >= 0; --bit) {
        G2Xyzz d;
        g2_dbl_impl(d, acc);
        acc = d;
        const uint32_t w = bit >= 32 ? G2_BN_X_HI : G2_BN_X_LO;
        if ((w >> (bit & 31)) & 1u) g2_madd<false>(acc, p, 0);
    }
    out = acc;
}

// a == b as points, both stored-form XYZZ, without an inversion: X1 ZZ2 == X2 ZZ1 and Y1 ZZZ2 == Y2 ZZZ1
KZG_HD bool g2_equal(const G2Xyzz& a, const G2Xyzz& b) {
    if (a.inf || b.inf) return a.inf && b.inf;
    Fq2 u1, u2, d, dd;
    fq2_mul(u1, a.x, b.zz);                    // 4 * 4
    fq2_mul(u2, b.x, a.zz);
    fq2_sub(d, u2, u1);                        // class O - class O: |.| < 1.01m
    fq2_sqr(dd, d);                            // class F; zero exactly when d is (Fq2 is a field)
    const bool ex = fq2_is_zero_mod(dd);
    fq2_mul(u1, a.y, b.zzz);
    fq2_mul(u2, b.y, a.zzz);
    fq2_sub(d, u2, u1);
    fq2_sqr(dd, d);
    const bool ey = fq2_is_zero_mod(dd);
    return ex && ey;
}

// P (affine, on the twist, not the identity) is in the order-r subgroup: [x + 1]P + psi([x]P) + psi^2([x]P) == psi^3([2x]P).
// One g2_mul_x, three psi, four additions (one of them the doubling on the right), one comparison.
KZG_HD bool g2_in_subgroup(const G2Affine& p) {
    G2Xyzz t, lhs;
    g2_mul_x(t, p);                            // [x]P
    lhs = t;
    g2_madd<false>(lhs, p, 0);                 // [x + 1]P
    g2_psi_xyzz(t);
    g2_add_into(lhs, t);                       // + psi([x]P)
    g2_psi_xyzz(t);
    g2_add_into(lhs, t);                       // + psi^2([x]P)
    g2_psi_xyzz(t);
    G2Xyzz rhs;
    { const G2Xyzz tc = t; g2_dbl(rhs, tc); } // psi^3([x]P) doubled = psi^3([2x]P)
    return g2_equal(lhs, rhs);
}

// out = [k]P for the low `bits` bits of k (8 little-endian words), P affine and not the identity: double-and-add from bit bits - 1
// down.  `bits` is uniform over a launch, so every lane runs the same trip count; bits = 0 gives the identity.
KZG_HD void g2_mul_bits(G2Xyzz& out, const G2Affine& p, const uint32_t k[8], int bits) {
    G2Xyzz acc;
    g2_set_inf(acc);
#pragma unroll 1
    for (int bit = bits - 1; bit >= 0; --bit) {
        G2Xyzz d;
        g2_dbl_impl(d, acc);
        acc = d;
        uint32_t w = k[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) w = (bit >> 5) == j ? k[j] : w;      // (a select chain: k stays in registers)
        if ((w >> (bit & 31)) & 1u) g2_madd<false>(acc, p, 0);
    }
    out = acc;
}

}  // namespace kzg
