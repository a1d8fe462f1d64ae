// pairing_dev.h — the optimal-ate pairing of BN254 for one lane of a device kernel (pairing.hip) and for the host check build
// (tests/hostcheck/pairingdevcheck.cpp): a product of Miller functions over up to ATE_CHUNK pairs with ONE squaring of f per step,
// one doubling and one addition line per pair, the two Frobenius addition steps, and fq12.h's final exponentiation.
//
// It restates host_pairing.h (ate_dbl_step, ate_add_step, mul_by_line, miller_ate_product; that file is the oracle and has the
// derivation of the lines): T in Jacobian coordinates on the twist, the line through T with slope lambda evaluated at P = (xP, yP) as
// a + b w + c w^3 with Fq2 coefficients scaled by a factor in Fq2 that the final exponentiation removes:
//   tangent at T = (X, Y, Z):  (Z3 Z^2) yP - (3 X^2 Z^2) xP w + (3 X^3 - 2 Y^2) w^3,          Z3 = 2 Y Z
//   chord through T and Q:     Z3 yP - r xP w + (r xQ - Z3 yQ) w^3,   H = xQ Z^2 - X, r = yQ Z^3 - Y, Z3 = H Z
// The same formulas give the same Miller value as the host's (an equality in Fq12, whatever the chunking: a product of Miller values
// with a shared squaring IS the Miller value of the pairs together), and the exponent is the host's, so GT values agree bit for bit.
// The degenerate rule is the host's too: an addition step that meets H == 0 (T == +-Q, only possible for a Q outside the order-r
// subgroup) sets *bad, and the caller's verdict is 0.
//
// STORED FORM of a pair's state: T.X, T.Y, T.Z and Q in class O of fq2.h; yP and -xP normalised in (-2m, 2m).  Bounds per line as in
// curve_g2.h: |component| in m, Karatsuba's (|a0| + |a1|)(|b0| + |b1|) in m^2 (< 169).
#pragma once
#include "curve_g2.h"
#include "fq12.h"

namespace kzg {

constexpr int ATE_CHUNK = 4;           // pairs of one shared loop (host_pairing.h's miller_ate_product holds 4 as well)

struct AteLine { Fq2 a, b, c; };       // a + b w + c w^3; a, b in class F, c in class O
struct AtePair {
    Fq2 X, Y, Z;                       // T
    Fq2 qx, qy;                        // Q
    Fq py, npx;                        // yP, -xP
};

// 8 c for a class-F c: normalised, |.| < 16m
KZG_HD void fq2_mul8(Fq2& r, const Fq2& c) {
    Fq2 t;
    fq2_dbl(t, c); fq2_dbl(t, t); fq2_norm(t);     // limbs up to 2^31 - 4
    fq2_dbl(t, t); fq2_norm(t);
    r = t;
}

// T <- 2 T (dbl-2009-l, a = 0) and the tangent at the old T evaluated at P
KZG_HD_NOINLINE void ate_dbl_step(AtePair& s, AteLine& l) {
    Fq2 A, B, C, D, E, Z2, X3, Y3, Z3, t, u;
    fq2_sqr(A, s.X);                           // 4.0; class F
    fq2_sqr(B, s.Y);
    fq2_sqr(C, B);                             // 16.0
    fq2_add(t, s.X, B); fq2_norm(t);           // (-1.0001m, 3.0001m)
    fq2_sqr(D, t);                             // 36.0
    fq2_sub(D, D, A); fq2_sub(D, D, C);        // (-5m, 4m), limbs in (-2^30, 2^29)
    fq2_reduce(D);
    fq2_dbl(D, D); fq2_norm(D);                // D = 2 ((X + B)^2 - A - C): (-0.0002m, 2.0002m)
    fq2_add(E, A, A); fq2_add(E, E, A); fq2_norm(E);       // E = 3 A: |.| < 6m
    fq2_sqr(Z2, s.Z);                          // 4.0
    fq2_sqr(X3, E);                            // 144.0
    fq2_dbl(t, D);                             // limbs below 2^30
    fq2_sub(X3, X3, t);                        // (-5.0004m, 2.0004m)
    fq2_reduce(X3);
    fq2_sub(t, D, X3);                         // (-1.0003m, 2.0003m), limbs within +-2^29
    fq2_mul_lazy(Y3, E, t);                    // 12 * 4.0006 = 48.0
    fq2_mul8(u, C);                            // |.| < 16m, limbs below 2^29
    fq2_sub(Y3, Y3, u);                        // (-21m, 12m), limbs above -2^31
    fq2_reduce(Y3);
    fq2_mul(Z3, s.Y, s.Z);                     // 4.0
    fq2_dbl(Z3, Z3);
    fq2_reduce(Z3);                            // Z3 = 2 Y Z, class O
    fq2_mul(t, Z3, Z2);                        // 2.0002 * 4
    fq2_mul_fq(l.a, t, s.py);                  // 1.0001 * 2; class F
    fq2_mul(t, E, Z2);                         // 12 * 4 = 48
    fq2_mul_fq(l.b, t, s.npx);                 // -(E Z^2) xP
    fq2_mul_lazy(t, E, s.X);                   // 12 * 2.0002
    fq2_dbl(u, B);                             // limbs below 2^30, |.| < 4m
    fq2_sub(t, t, u);                          // (-9m, 6m)
    fq2_reduce(t);
    l.c = t;                                   // E X - 2 B
    s.X = X3; s.Y = Y3; s.Z = Z3;
}

// T <- T + Q for an affine Q in class O (madd) and the chord through the old T and Q evaluated at P.  false: H == 0, T == +-Q (the
// degenerate case of host_pairing.h's ate_add_step): T and l are left as they are.
KZG_HD_NOINLINE bool ate_add_step(AtePair& s, const Fq2& qx, const Fq2& qy, AteLine& l) {
    Fq2 Z2, H, r, Z3, HH, HHH, V, X3, Y3, t, u;
    fq2_sqr(Z2, s.Z);                          // 4.0
    fq2_mul(H, qx, Z2);                        // 2.0002 * 4
    fq2_sub(H, H, s.X);                        // |.| < 1.0002m
    fq2_reduce(H);                             // class O: inside fq2_is_zero_mod's class F
    if (fq2_is_zero_mod(H)) return false;
    fq2_mul(t, Z2, s.Z);                       // 4 * 2.0002
    fq2_mul(r, qy, t);
    fq2_sub(r, r, s.Y);
    fq2_reduce(r);                             // r = yQ Z^3 - Y, class O
    fq2_mul(Z3, s.Z, H);                       // 4.0
    fq2_mul_fq(l.a, Z3, s.py);
    fq2_mul_fq(l.b, r, s.npx);                 // -r xP
    fq2_mul_lazy(t, r, qx);                    // 4.0
    fq2_mul_lazy(u, Z3, qy);
    fq2_sub(t, t, u);                          // c0 in (-6m, 6m), c1 in (-9m, 9m); limbs within +-(2^30 + 2^29)
    fq2_reduce(t);
    l.c = t;                                   // r xQ - Z3 yQ
    fq2_sqr(HH, H);                            // 4.0
    fq2_mul(HHH, H, HH);                       // 2.0002 * 4
    fq2_mul(V, s.X, HH);
    fq2_sqr(X3, r);                            // 4.0
    fq2_sub(X3, X3, HHH); fq2_sub(X3, X3, V); fq2_sub(X3, X3, V);      // (-4.0003m, 2.0001m), limbs above -(2^30 + 2^29)
    fq2_reduce(X3);
    fq2_sub(t, V, X3);                         // |.| < 1.0002m
    fq2_mul_lazy(Y3, r, t);                    // 2.0002 * 2.0004
    fq2_mul_lazy(u, s.Y, HHH);                 // 4.0
    fq2_sub(Y3, Y3, u);
    fq2_reduce(Y3);
    s.X = X3; s.Y = Y3; s.Z = Z3;
    return true;
}

// f (a + b w + c w^3): h_k = a g_k + b g'_(k-1) + c g'_(k-3), the index wrapping through w^6 = xi (g'_j = xi g_(j+6) for j < 0).
// 18 lazy products = 54 Fq products.  a, b class F and c class O: 4; g_j 2.0002, xi g_j 20.002: 8.0 and 80.0.  Sum of three: 15m, reduced.
KZG_HD_NOINLINE void fq12_mul_by_line(Fq12& f, const AteLine& l) {
    Fq2 xg[6];
#pragma unroll 1
    for (int j = 3; j < 6; ++j) fq2_mul_xi(xg[j], f.g[j]);
    Fq12 h;
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        const Fq2* gb = k >= 1 ? &f.g[k - 1] : &xg[5];
        const Fq2* gc = k >= 3 ? &f.g[k - 3] : &xg[k + 3];
        Fq2 acc, p;
        fq2_mul_lazy(acc, l.a, f.g[k]);
        fq2_norm(acc);
        fq2_mul_lazy(p, l.b, *gb);
        fq2_acc(acc, p);
        fq2_mul_lazy(p, l.c, *gc);
        fq2_acc(acc, p);
        fq2_reduce(acc);
        h.g[k] = acc;
    }
    f = h;
}

// pi(Q) and -pi^2(Q) on the twist (host_pairing.h g2_frobenius, g2_frobenius2_neg), class O
KZG_HD void ate_frobenius_points(Fq2& x1, Fq2& y1, Fq2& x2, const Fq2& qx, const Fq2& qy, const PairingConsts& C) {
    Fq2 k, c;
    fq2_unpack(k, C.twist_frob_x);
    c = qx; fe_neg(c.c1, c.c1); fe_norm(c.c1);
    fq2_mul(x1, c, k);                         // 2.0002 * 2
    fq2_unpack(k, C.twist_frob_y);
    c = qy; fe_neg(c.c1, c.c1); fe_norm(c.c1);
    fq2_mul(y1, c, k);
    Fq k2;
    fe_unpack(k2, C.twist_frob2_x);
    fq2_mul_fq(x2, qx, k2);                    // class F
    fq2_reduce(x2);
}

// the state of a pair at the start of a loop: T = Q; x, y of P in class F (fe_from_wire / fe_unpack), Q in class O
KZG_HD void ate_pair_init(AtePair& s, const Fq& px, const Fq& py, const Fq2& qx, const Fq2& qy) {
    s.X = qx; s.Y = qy; fq2_set_one(s.Z);
    s.qx = qx; s.qy = qy;
    s.py = py;
    fe_neg(s.npx, px); fe_norm(s.npx);         // (-2m, m)
}

// f = prod_k f_(6x+2, Q_k)(P_k) l l' over m <= ATE_CHUNK pairs, none of them with an identity point (the caller skips those).
// *bad |= an addition step was degenerate: f then has no meaning.
KZG_HD_NOINLINE void miller_ate_product_dev(Fq12& f, AtePair* pts, int m, const PairingConsts& C, bool* bad) {
    fq12_set_one(f);
    AteLine l;
#pragma unroll 1
    for (int i = C.naf_len - 2; i >= 0; --i) {
        fq12_sqr(f, f);
#pragma unroll 1
        for (int k = 0; k < m; ++k) { ate_dbl_step(pts[k], l); fq12_mul_by_line(f, l); }
        const int d = C.naf[i];
        if (d) {
#pragma unroll 1
            for (int k = 0; k < m; ++k) {
                Fq2 qy = pts[k].qy;
                if (d < 0) fq2_neg_stored(qy, qy);
                const Fq2 qx = pts[k].qx;
                if (ate_add_step(pts[k], qx, qy, l)) fq12_mul_by_line(f, l); else *bad = true;
            }
        }
    }
#pragma unroll 1
    for (int k = 0; k < m; ++k) {
        Fq2 x1, y1, x2;
        ate_frobenius_points(x1, y1, x2, pts[k].qx, pts[k].qy, C);
        if (ate_add_step(pts[k], x1, y1, l)) fq12_mul_by_line(f, l); else *bad = true;
        const Fq2 qy = pts[k].qy;
        if (ate_add_step(pts[k], x2, qy, l)) fq12_mul_by_line(f, l); else *bad = true;
    }
}

// ---------------------------------------------------------------------------------------------
// Points of a check.  G1: device affine format of curve.h (16 u32), G2: that of curve_g2.h (32 u32); the identity is all zero.
// ---------------------------------------------------------------------------------------------
// y^2 == x^3 + 3 for coordinates in class F
KZG_HD bool g1_on_curve_dev(const Fq& x, const Fq& y) {
    Fq t, y2, b3;
#pragma unroll
    for (int j = 0; j < NL; ++j) b3.l[j] = (int32_t)FqParams::B3[j];
    fe_sqr(t, x);
    fe_mul(t, t, x);
    fe_add(t, t, b3);
    fe_norm(t);                                // x^3 + 3, |.| < 4m
    fe_sqr(y2, y);
    fe_sub(t, y2, t);
    fe_reduce_small(t);
    return fe_is_zero_mod(t);
}
// one pair from its wire words to the two device formats; flags: 1 = the G1 point is off the curve, 2 = the G2 point is off the twist
KZG_HD uint32_t pairing_pair_to_device(uint32_t g1_dev[16], uint32_t g2_dev[32], const uint32_t g1_wire[16], const uint32_t g2_wire[32]) {
    uint32_t flags = 0, any = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) any |= g1_wire[j];
    Fq x, y;
    fe_from_wire(x, g1_wire);
    fe_from_wire(y, g1_wire + 8);
    if (any && !g1_on_curve_dev(x, y)) flags |= 1;
    fe_canon(x); fe_canon(y);
    fe_pack(g1_dev, x); fe_pack(g1_dev + 8, y);
    bool on_twist;
    g2_affine_wire_to_device(g2_dev, g2_wire, &on_twist);
    if (!on_twist) flags |= 2;
    return flags;
}

// One check: the pairs [lo, hi) of the two device-format arrays; pairs with an identity point contribute 1, the others run in
// chunks of ATE_CHUNK whose Miller values are multiplied before the ONE final exponentiation.  gt: the 96 flat wire words of the
// value (all zero when a step was degenerate: no GT element).  Returns the verdict: not degenerate and the value is 1.
KZG_HD_NOINLINE bool pairing_check_dev(uint32_t gt[96], const uint32_t* g1_dev, const uint32_t* g2_dev, uint32_t lo, uint32_t hi, const PairingConsts& C) {
    AtePair pts[ATE_CHUNK];
    Fq12 acc, f;
    bool have = false, bad = false;
    uint32_t k = lo;
#pragma unroll 1
    while (k < hi) {
        int m = 0;
#pragma unroll 1
        for (; k < hi && m < ATE_CHUNK; ++k) {
            const uint32_t* p = g1_dev + 16 * (size_t)k;
            const uint32_t* q = g2_dev + 32 * (size_t)k;
            uint32_t anyp = 0, anyq = 0;
#pragma unroll 1
            for (int j = 0; j < 16; ++j) anyp |= p[j];
#pragma unroll 1
            for (int j = 0; j < 32; ++j) anyq |= q[j];
            if (!anyp || !anyq) continue;
            Fq px, py;
            Fq2 qx, qy;
            fe_unpack(px, p); fe_unpack(py, p + 8);
            fq2_unpack(qx, q); fq2_unpack(qy, q + 16);
            ate_pair_init(pts[m], px, py, qx, qy);
            ++m;
        }
        if (m == 0) break;
        miller_ate_product_dev(f, pts, m, C, &bad);
        if (have) fq12_mul(acc, acc, f); else acc = f;
        have = true;
    }
    if (bad) {
#pragma unroll 1
        for (int j = 0; j < 96; ++j) gt[j] = 0;
        return false;
    }
    if (have) fq12_final_exponentiation(acc, acc, C); else fq12_set_one(acc);
    fq12_to_flat_wire(gt, acc);
    return fq12_wire_is_one(gt);
}

}  // namespace kzg
