// fq12.h — Fq12 for the device pairing (pairing_dev.h) over the signed 9 x 29-bit Fq of field29.h and the Fq2 of fq2.h.
//
// An element is six Fq2 coefficients g_i of w^i with w^6 = xi = 9 + u:  Fq12 = Fq2[w] / (w^6 - xi).  host_pairing.h writes the same
// field as twelve Fq coefficients c_i of Fq[w] / (w^12 - 18 w^6 + 82) and switches to this form for its line products and its
// cyclotomic squarings (g_i = (c_i + 9 c_(i+6)) + c_(i+6) u); here it is the only form, and the flat one exists at the wire
// (fq12_from_flat_wire / fq12_to_flat_wire), so that GT values compare bit for bit with the host's.
//
// STORED FORM of an Fq12 (what every function below leaves): all twelve components in class O of fq2.h, normalised and in
// (-0.0001m, 1.0001m).  Operands may be anywhere in class F, (-m, 2m), normalised: the products then stand at 4 * 40 = 160 m^2, still
// inside the bound; the annotations give the figures for stored operands.  Every formula ends in one fq2_reduce per coefficient and is
// annotated with the value it reduces (in m) and with Karatsuba's requirement (|a0| + |a1|)(|b0| + |b1|) < 169 m^2 as its value in m^2,
// as fq2.h and curve_g2.h do; the
// KZG_BOUND_CHECK host build (tests/hostcheck/pairingdevcheck.cpp) and the KZG_DEVICE_BOUND_CHECK build check every one of them
// through the sites of fe_* / fq2_*: there is no site of this file's own.
//
// int32 limbs: a normalised limb is below 2^29, so at most three normalised values may be added before fe_norm (4 x 2^29 = 2^31),
// and a lazy Karatsuba result (limbs in (-2^30, 2^29)) may be added to ONE normalised value.  Hence the accumulations below
// normalise after every addition (27 instructions against the ~650 of the product they follow).
//
// WHERE AN Fq12 LIVES.  108 limbs: with two operands, a result and a Karatsuba product in flight nothing else fits the 512-entry
// register file, and a pairing holds about ten of them.  They are plain objects in PRIVATE memory (scratch), indexed at run time, and
// the products are loops over those indices around ONE inlined fq2 product: the functions are out of line (KZG_HD_NOINLINE, as the G2
// chain kernels keep g2_add out of line), so the code stays a few thousand instructions and compiles in seconds.  Scratch is
// interleaved by lane, so the 36 limb loads of an operand are coalesced dword loads that hit L1/L2; per Fq2 product they are 72
// loads beside ~650 VALU instructions.  profiles/pairing_device.md has the compiler's figures.
#pragma once
#include "fq2.h"

namespace kzg {

struct Fq12 {
    Fq2 g[6];
};

// Frobenius coefficients (w^i)^(p^k) / w^i in Fq2 for k = 1..3, i = 1..5 and the constants of the two Frobenius addition steps, as
// canonical residues of the internal Montgomery form (fe_pack's words): computed on the host from host_pairing.h's own tables
// (host_pairing_batch.h pairing_consts_build) and uploaded once per device; never typed in.
struct PairingConsts {
    uint32_t frob[3][5][16];       // [k - 1][i - 1] = c0[8] | c1[8]
    uint32_t twist_frob_x[16];     // pi(Q) = (conj(x) twist_frob_x, conj(y) twist_frob_y)
    uint32_t twist_frob_y[16];
    uint32_t twist_frob2_x[8];     // -pi^2(Q) = (x twist_frob2_x, y)
    int32_t naf_len;               // signed digits of 6x + 2, least significant first
    int32_t naf[67];
};

KZG_HD void fq12_set_one(Fq12& r) {
    fq2_set_one(r.g[0]);
#pragma unroll 1
    for (int i = 1; i < 6; ++i) fq2_set_zero(r.g[i]);
}

// 9 a for a normalised a: normalised.  Limbs: 4 a_j <= 2^31 - 4 (fits, and stays inside int32 with the carries of fe_norm), then
// 2 (..) + a_j < 2^30 + 2^29.
KZG_HD void fe_mul9(Fq& r, const Fq& a) {
    Fq t;
    fe_dbl(t, a); fe_dbl(t, t); fe_norm(t);
    fe_dbl(t, t); fe_add(t, t, a); fe_norm(t);
    r = t;
}
// xi a = (9 a0 - a1) + (9 a1 + a0) u for a normalised a with |a_i| < A m: normalised, |.| < 10 A m
KZG_HD void fq2_mul_xi(Fq2& r, const Fq2& a) {
    Fq n0, n1;
    fe_mul9(n0, a.c0); fe_mul9(n1, a.c1);
    fe_sub(n0, n0, a.c1); fe_norm(n0);
    fe_add(n1, n1, a.c0); fe_norm(n1);
    r.c0 = n0; r.c1 = n1;
}
// acc += p for a normalised acc and a lazy product p (limbs in (-2^30, 2^29)): limbs within +-2^30 before the normalisation
KZG_HD void fq2_acc(Fq2& acc, const Fq2& p) { fq2_add(acc, acc, p); fq2_norm(acc); }

// a b.  h_k = sum_{i <= k} a_i b_(k-i) + sum_{i > k} a_i (xi b)_(k+6-i): six lazy products per coefficient, 36 in all = 108 Fq
// products (the host's one-level Karatsuba over the flat form costs the same 108).
// Operands stored form: a_i: 2.0002; b_j: 2.0002, xi b_j: |.| < 10.001m so 20.002: products 4.0 and 40.01.  Sum of six lazy
// results: |.| < 6 * 5m = 30m, reduced once.
KZG_HD_NOINLINE void fq12_mul(Fq12& r, const Fq12& a, const Fq12& b) {
    Fq2 xb[6];
#pragma unroll 1
    for (int j = 1; j < 6; ++j) fq2_mul_xi(xb[j], b.g[j]);
    Fq12 t;
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        Fq2 acc;
        fq2_set_zero(acc);
#pragma unroll 1
        for (int i = 0; i < 6; ++i) {
            const Fq2* bj = i <= k ? &b.g[k - i] : &xb[k + 6 - i];
            Fq2 p;
            fq2_mul_lazy(p, a.g[i], *bj);
            fq2_acc(acc, p);
        }
        fq2_reduce(acc);                       // 30m -> class O
        t.g[k] = acc;
    }
    r = t;
}

// a^2: the products a_i a_j, i < j, once and doubled (15 of them), the six squares as a_i (a_i or xi a_i): 21 lazy products = 63 Fq
// products, the host's count.  Per coefficient at most three doubled products and two squares: 2 * 3 * 5m + 2 * 5m = 40m.
KZG_HD_NOINLINE void fq12_sqr(Fq12& r, const Fq12& a) {
    Fq2 xa[6];
#pragma unroll 1
    for (int j = 1; j < 6; ++j) fq2_mul_xi(xa[j], a.g[j]);
    Fq12 t;
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        Fq2 cross, diag;
        fq2_set_zero(cross); fq2_set_zero(diag);
#pragma unroll 1
        for (int i = 0; i < 6; ++i) {
            const int j = i <= k ? k - i : k + 6 - i;
            if (i > j) continue;
            const Fq2* aj = i <= k ? &a.g[j] : &xa[j];
            Fq2 p;
            fq2_mul_lazy(p, a.g[i], *aj);      // 4.0 / 40.01
            if (i < j) fq2_acc(cross, p); else fq2_acc(diag, p);
        }
        fq2_dbl(cross, cross);                 // normalised, |.| < 15m: limbs below 2^30, |.| < 30m
        fq2_add(cross, cross, diag);           // + normalised, |.| < 10m: limbs below 2^30 + 2^29, |.| < 40m
        fq2_reduce(cross);
        t.g[k] = cross;
    }
    r = t;
}

// a (c0 + c1 u): every coefficient times one Fq2 (the inverse of the norm in fq12_inverse).  s in class F: 2.0002 * 4
KZG_HD void fq12_mul_fq2(Fq12& r, const Fq12& a, const Fq2& s) {
#pragma unroll 1
    for (int i = 0; i < 6; ++i) { Fq2 t; fq2_mul(t, a.g[i], s); r.g[i] = t; }
}

// -a in the stored form: the negation of a class-O value lies in (-1.0001m, 0.0001m); reduced back into class O
KZG_HD void fq2_neg_stored(Fq2& r, const Fq2& a) {
    Fq2 t;
    fq2_neg(t, a);
    fq2_reduce(t);
    r = t;
}
// a^(p^6): w -> -w, the odd coefficients change sign.  In the cyclotomic subgroup this is the inverse.  r may be a
KZG_HD void fq12_conj(Fq12& r, const Fq12& a) {
#pragma unroll 1
    for (int i = 0; i < 6; ++i) {
        if (i & 1) fq2_neg_stored(r.g[i], a.g[i]);
        else { Fq2 t = a.g[i]; fq2_reduce(t); r.g[i] = t; }         // (a class-F operand leaves in class O as well)
    }
}

// a^(p^k), k = 1..3: g_i w^i -> conj^k(g_i) gamma_(k,i) w^i with gamma_(k,i) = (w^i)^(p^k) / w^i in Fq2 (PairingConsts::frob; gamma_(k,0) = 1).
// conj(g_i) lies in (-1.0001m, 1.0001m) with limbs within +-2^29: 2.0002 * 2 (the table is canonical).  r may be a
KZG_HD_NOINLINE void fq12_frobenius(Fq12& r, const Fq12& a, int k, const PairingConsts& C) {
#pragma unroll 1
    for (int i = 0; i < 6; ++i) {
        Fq2 c = a.g[i];
        if (k & 1) { fe_neg(c.c1, c.c1); fe_norm(c.c1); }
        if (i) {
            Fq2 gam;
            fq2_unpack(gam, C.frob[k - 1][i - 1]);
            fq2_mul(c, c, gam);
        } else {
            fq2_reduce(c);
        }
        r.g[i] = c;
    }
}

// (a + b s)^2 = (a^2 + xi b^2) + 2 a b s in Fq4 = Fq2[s] / (s^2 - xi); a, b class O.  c0 = t0 + xi t1: t1 class F so |xi t1| < 20m, 22m
// reduced; c1 = (a + b)^2 - t0 - t1: the sum has |.| < 2.0002m, (4.0004)^2 = 16; (-5m, 4m) reduced.
KZG_HD void fq4_sqr(Fq2& c0, Fq2& c1, const Fq2& a, const Fq2& b) {
    Fq2 t0, t1, s, x;
    fq2_sqr(t0, a); fq2_sqr(t1, b);            // 4.0
    fq2_add(s, a, b); fq2_norm(s);
    fq2_sqr(s, s);                             // 16.0
    fq2_sub(s, s, t0); fq2_sub(s, s, t1);
    fq2_reduce(s);
    fq2_mul_xi(x, t1);
    fq2_add(x, x, t0);                         // limbs below 2^30
    fq2_reduce(x);
    c0 = x; c1 = s;
}
// 3 t + 2 z (sign = +1) or 3 t - 2 z (sign = -1) for a normalised t with |t| < T m and a class-O z: 2 (t +- z) + t, (3 T + 2.0002) m, reduced
KZG_HD void fq2_three_two(Fq2& r, const Fq2& t, const Fq2& z, int sign) {
    Fq2 s;
    if (sign > 0) fq2_add(s, t, z); else fq2_sub(s, t, z);
    fq2_norm(s);
    fq2_dbl(s, s);                             // limbs below 2^30
    fq2_add(s, s, t);                          // below 2^30 + 2^29
    fq2_reduce(s);
    r = s;
}
// Squaring in the cyclotomic subgroup (Granger-Scott; host_pairing.h cyclotomic_sqr): three squarings in Fq4, nine Fq2 squarings.
// With the tower's names z0 = g0, z4 = g2, z3 = g4, z2 = g1, z1 = g3, z5 = g5.  r may be a (every z is read before a g is written).
KZG_HD_NOINLINE void fq12_cyclotomic_sqr(Fq12& r, const Fq12& a) {
    Fq2 t0, t1, t2, t3, t4, t5, x;
    fq4_sqr(t0, t1, a.g[0], a.g[3]);
    fq4_sqr(t2, t3, a.g[1], a.g[4]);
    fq4_sqr(t4, t5, a.g[2], a.g[5]);
    const Fq2 z0 = a.g[0], z1 = a.g[3], z2 = a.g[1], z3 = a.g[4], z4 = a.g[2], z5 = a.g[5];
    fq2_three_two(r.g[0], t0, z0, -1);         // 3 * 1.0001 + 2.0002
    fq2_three_two(r.g[3], t1, z1, +1);
    fq2_mul_xi(x, t5);                         // |.| < 10.001m
    fq2_three_two(r.g[1], x, z2, +1);          // 3 * 10.001 + 2.0002 = 32.01m
    fq2_three_two(r.g[4], t4, z3, -1);
    fq2_three_two(r.g[2], t2, z4, -1);
    fq2_three_two(r.g[5], t3, z5, +1);
}

// a^x for the BN parameter x = 4965661367192848881 (63 bits) and a in the cyclotomic subgroup: 62 cyclotomic squarings, 27 products
KZG_HD_NOINLINE void fq12_pow_x(Fq12& r, const Fq12& a) {
    const uint64_t X = 0x44e992b44a6909f1ULL;
    Fq12 acc = a;
#pragma unroll 1
    for (int i = 61; i >= 0; --i) {
        fq12_cyclotomic_sqr(acc, acc);
        if ((X >> i) & 1) fq12_mul(acc, acc, a);
    }
    r = acc;
}

// 1 / f through norms (host_pairing.h fq12_inverse_norm): g = f conj(f) lies in Fq6, d = g g^(p^2) g^(p^4) in Fq2 -- here simply
// the coefficient of w^0 --, so 1 / f = conj(f) g^(p^2) g^(p^4) / d with ONE inversion in Fq.  false: f == 0
KZG_HD_NOINLINE bool fq12_inverse(Fq12& r, const Fq12& f, const PairingConsts& C) {
    Fq12 fbar, g, g2, g4;
    fq12_conj(fbar, f);
    fq12_mul(g, f, fbar);
    fq12_frobenius(g2, g, 2, C);
    fq12_frobenius(g4, g2, 2, C);
    fq12_mul(g2, g2, g4);                      // t = g^(p^2) g^(p^4)
    fq12_mul(g, g, g2);                        // d
    const Fq2 d = g.g[0];                      // class O, inside class F
    if (fq2_is_zero_mod(d)) return false;
    Fq2 di;
    fq2_inv(di, d);                            // class F
    fq12_mul(g2, fbar, g2);
    fq12_mul_fq2(r, g2, di);
    return true;
}

// f^((p^12 - 1) / r) with host_pairing.h's final_exponentiation_x, line by line: the easy part (p^6 - 1)(p^2 + 1), three powers by x and
// the vector addition chain y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36 (Scott et al. 2009).  The exponent is the host's, so GT values are the
// host's bit for bit.  f == 0 (no valid input gives it) returns f, as the host does.
KZG_HD_NOINLINE void fq12_final_exponentiation(Fq12& r, const Fq12& f, const PairingConsts& C) {
    Fq12 g, fx, fx2, fx3, t0, t1, u, v;
    if (!fq12_inverse(u, f, C)) { r = f; return; }
    fq12_conj(g, f);
    fq12_mul(g, g, u);                         // f^(p^6 - 1)
    fq12_frobenius(u, g, 2, C);
    fq12_mul(g, u, g);                         // ^(p^2 + 1)
    fq12_pow_x(fx, g);
    fq12_pow_x(fx2, fx);
    fq12_pow_x(fx3, fx2);
    fq12_frobenius(u, fx3, 1, C); fq12_mul(u, fx3, u); fq12_conj(u, u);      // y6
    fq12_sqr(t0, u);
    fq12_frobenius(u, fx2, 1, C); fq12_mul(u, fx, u); fq12_conj(u, u);       // y4
    fq12_mul(t0, t0, u);
    fq12_conj(v, fx2);                                                       // y5
    fq12_mul(t0, t0, v);
    fq12_frobenius(u, fx, 1, C); fq12_conj(u, u);                            // y3
    fq12_mul(t1, u, v);
    fq12_mul(t1, t1, t0);
    fq12_frobenius(u, fx2, 2, C);                                            // y2
    fq12_mul(t0, t0, u);
    fq12_sqr(t1, t1);
    fq12_mul(t1, t1, t0);
    fq12_sqr(t1, t1);
    fq12_conj(u, g);                                                         // y1
    fq12_mul(t0, t1, u);
    fq12_frobenius(u, g, 1, C); fq12_frobenius(v, g, 2, C); fq12_mul(u, u, v);
    fq12_frobenius(v, g, 3, C); fq12_mul(u, u, v);                           // y0
    fq12_mul(t1, t1, u);
    fq12_sqr(t0, t0);
    fq12_mul(r, t0, t1);
}

// ---------------------------------------------------------------------------------------------
// The flat form at the wire: 12 x 8 u32, coefficient c_i of the host's Fq[w] / (w^12 - 18 w^6 + 82), arkworks Montgomery words.
//   g_i = (c_i + 9 c_(i+6)) + c_(i+6) u,   c_i = g_i.c0 - 9 g_i.c1,  c_(i+6) = g_i.c1
// ---------------------------------------------------------------------------------------------
KZG_HD void fq12_from_flat_wire(Fq12& r, const uint32_t w[96]) {
#pragma unroll 1
    for (int i = 0; i < 6; ++i) {
        Fq lo, hi, n;
        fe_from_wire(lo, w + 8 * i);           // (-m, 2m)
        fe_from_wire(hi, w + 8 * (i + 6));
        fe_mul9(n, hi);                        // |.| < 18m
        fe_add(lo, lo, n);                     // limbs below 2^30, |.| < 20m
        r.g[i].c0 = lo; r.g[i].c1 = hi;
        fq2_reduce(r.g[i]);
    }
}
KZG_HD void fq12_to_flat_wire(uint32_t w[96], const Fq12& a) {
#pragma unroll 1
    for (int i = 0; i < 6; ++i) {
        Fq n, lo;
        fe_mul9(n, a.g[i].c1);                 // |.| < 9.001m
        fe_sub(lo, a.g[i].c0, n); fe_norm(lo); // |.| < 10.01m: inside fe_to_wire's 169m
        fe_to_wire(w + 8 * i, lo);
        fe_to_wire(w + 8 * (i + 6), a.g[i].c1);
    }
}
// a == 1, decided on the canonical wire words (what the host's fq12_is_one compares)
KZG_HD bool fq12_wire_is_one(const uint32_t w[96]) {
    Fq one;
    fe_set_one(one);
    uint32_t ow[8];
    fe_to_wire(ow, one);
    uint32_t diff = 0;
#pragma unroll 1
    for (int j = 0; j < 96; ++j) diff |= w[j] ^ (j < 8 ? ow[j] : 0u);
    return diff == 0;
}

}  // namespace kzg
