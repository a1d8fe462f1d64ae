// curve_g2.h — BN254 G2 (the twist y^2 = x^3 + 3 / (9 + u) over Fq2, fq2.h) group law in extended Jacobian ("XYZZ") coordinates:
// x = X / ZZ, y = Y / ZZZ, ZZ^3 = ZZZ^2.  The formulas are those of curve.h (madd-2008-s, mdbl / dbl-2008-s-1, add-2008-s) with Fq2
// coordinates; a = 0 on the twist too, so no formula multiplies by the twist constant: only the on-twist check adds it.
//
// This is the arithmetic behind the protocol's two G2 multi-scalar multiplications (length commitment sum f_i [tau^i]_2 and length
// proof sum f_i [tau^(N-d+i)]_2), which the reference takes with `G2Projective::msm`.
//
// Every exceptional case is explicit: identity accumulator, identity base (callers skip it: g2_affine_load returns false), P + P,
// P + (-P), and -- G2 only -- a point of order two (y == 0: the twist's group has a cofactor and uploads do not check the subgroup),
// whose double is the identity.
//
// Stored form of an XYZZ value (registers or memory): all eight Fq components NORMALISED and in (-m, 2m) (class F of fq2.h); the
// identity is flagged by `inf` in registers and by ZZ == literal 0 in memory.  Affine points are canonical, [0, m).
// Bounds are annotated per line as |component| and the Karatsuba requirement (|a0| + |a1|)(|b0| + |b1|) < 169 m^2 as its value in
// m^2; the KZG_BOUND_CHECK host build and the KZG_DEVICE_BOUND_CHECK build verify them.
#pragma once
#include "curve.h"      // uint4 of the host-check build
#include "fq2.h"

namespace kzg {

struct G2Affine {      // unpacked affine point, coordinates canonical in [0, m) (internal Montgomery)
    Fq2 x, y;
};

struct G2Xyzz {
    Fq2 x, y, zz, zzz;
    bool inf;
};

constexpr int G2_LIMBS = 8 * NL;       // limb planes of a stored XYZZ value

KZG_HD void g2_set_inf(G2Xyzz& r) {
    fq2_set_zero(r.x); fq2_set_zero(r.y); fq2_set_zero(r.zz); fq2_set_zero(r.zzz);
    r.inf = true;
}

// r = (x, +-y) as XYZZ
KZG_HD void g2_from_affine(G2Xyzz& r, const G2Affine& p, uint32_t neg) {
    r.x = p.x;
    fq2_cneg(r.y, p.y, neg);
    fq2_norm(r.y);                             // stored form: (-m, m), limbs 0..7 non-negative
    fq2_set_one(r.zz);
    fq2_set_one(r.zzz);
    r.inf = false;
}

// X3 = M^2 - 2 S, Y3 = M (S - X3) - W Y: the tail shared by both doublings.  M: |M_i| < 6m; S, W in class O; y: |y_i| < 2m.
KZG_HD void g2_dbl_tail(Fq2& x3, Fq2& y3, const Fq2& m, const Fq2& s, const Fq2& w, const Fq2& y) {
    Fq2 t, a, b;
    fq2_sqr(x3, m);                            // 12 * 12 = 144 m^2
    fq2_sub(x3, x3, s); fq2_sub(x3, x3, s);    // (-3.01m, 2.01m)
    fq2_reduce(x3);                            // class O
    fq2_sub(t, s, x3);                         // |.| < 1.01m, limbs within +-2^29
    fq2_mul_lazy(a, m, t);                     // 12 * 2.02
    fq2_mul_lazy(b, w, y);                     // 2.02 * 4
    fq2_sub(y3, a, b);                         // c0 in (-6m, 6m), c1 in (-9m, 9m); limbs within +-(2^30 + 2^29)
    fq2_reduce(y3);                            // class O
}

// Doubling of an affine point (mdbl-2008-s-1 with ZZ = ZZZ = 1).  y2 already carries the sign, |y2_i| < m.
KZG_HD void g2_dbl_affine_impl(G2Xyzz& r, const Fq2& x2, const Fq2& y2) {
    Fq2 u, v, w, s, m, xx;
    fq2_dbl(u, y2); fq2_norm(u);               // |u_i| < 2m
    fq2_sqr(v, u);                             // V = U^2: 4 * 4
    if (fq2_is_zero_mod(v)) { g2_set_inf(r); return; }       // y == 0: a point of order two
    fq2_mul(w, u, v);                          // W = U V: 4 * 4
    fq2_mul(s, x2, v);                         // S = X V: 2 * 4
    fq2_sqr(xx, x2);
    fq2_add(m, xx, xx); fq2_add(m, m, xx); fq2_norm(m);      // M = 3 X^2, |M_i| < 6m
    g2_dbl_tail(r.x, r.y, m, s, w, y2);
    r.zz = v;
    r.zzz = w;
    r.inf = false;
}
KZG_HD_NOINLINE void g2_dbl_affine(G2Xyzz& r, const Fq2& x2, const Fq2& y2) { g2_dbl_affine_impl(r, x2, y2); }

// Doubling of a stored XYZZ value (dbl-2008-s-1).
KZG_HD void g2_dbl_impl(G2Xyzz& r, const G2Xyzz& p) {
    if (p.inf) { r = p; return; }
    Fq2 u, v, w, s, m, xx, x3, y3, zz3, zzz3;
    fq2_dbl(u, p.y); fq2_norm(u);              // |u_i| < 4m
    fq2_sqr(v, u);                             // 8 * 8 = 64
    if (fq2_is_zero_mod(v)) { g2_set_inf(r); return; }       // Y == 0: a point of order two
    fq2_mul(w, u, v);                          // 8 * 4
    fq2_mul(s, p.x, v);                        // 4 * 4
    fq2_sqr(xx, p.x);                          // 4 * 4
    fq2_add(m, xx, xx); fq2_add(m, m, xx); fq2_norm(m);      // |M_i| < 6m
    g2_dbl_tail(x3, y3, m, s, w, p.y);
    fq2_mul(zz3, v, p.zz);                     // 4 * 4
    fq2_mul(zzz3, w, p.zzz);                   // 2.02 * 4
    r.x = x3; r.y = y3; r.zz = zz3; r.zzz = zzz3; r.inf = false;
}
KZG_HD_NOINLINE void g2_dbl(G2Xyzz& r, const G2Xyzz& p) { g2_dbl_impl(r, p); }

// X3 = RR - PPP - 2 Q, Y3 = R (Q - X3) - S1 PPP: the tail shared by the mixed and the full addition.
// RR in class F; PPP, Q in class O; |R_i| < 3m; s1 in class F.
KZG_HD void g2_add_tail(Fq2& x3, Fq2& y3, const Fq2& rr, const Fq2& ppp, const Fq2& q, const Fq2& R, const Fq2& s1) {
    Fq2 v, t, a, b;
    fq2_sub(v, rr, ppp); fq2_sub(v, v, q); fq2_sub(v, v, q);     // (-4.01m, 2.01m)
    fq2_reduce(v);                             // class O
    fq2_sub(t, q, v);                          // |.| < 1.01m, limbs within +-2^29
    fq2_mul_lazy(a, R, t);                     // 6 * 2.02
    fq2_mul_lazy(b, s1, ppp);                  // 4 * 2.02
    fq2_sub(y3, a, b);                         // c0 in (-6m, 6m), c1 in (-9m, 9m)
    fq2_reduce(y3);                            // class O
    x3 = v;
}

// acc += (neg ? -p : p), p affine and NOT the identity (callers skip identity bases).   madd-2008-s, the CHECKED form: P == +-Q is
// tested on every addition (PP == 0 in Fq2, a field: exactly when P == 0).  8 Fq2 products + 2 squarings = 28 Fq products.
// INLINE_SLOW as in curve.h: true keeps the doubling inside the caller, false calls the out-of-line copy.
template <bool INLINE_SLOW = false>
KZG_HD void g2_madd(G2Xyzz& acc, const G2Affine& p, uint32_t neg) {
    if (acc.inf) { g2_from_affine(acc, p, neg); return; }
    Fq2 y2s, u2, s2, P, R, pp_, rr_, ppp, q, x3, y3, zz3, zzz3;
    fq2_cneg(y2s, p.y, neg);                   // |.| < m, limbs within +-2^29
    fq2_mul(u2, p.x, acc.zz);                  // U2 = x2 ZZ1: 2 * 4
    fq2_mul(s2, y2s, acc.zzz);                 // S2 = y2 ZZZ1: 2 * 4
    fq2_sub(P, u2, acc.x);                     // class O - class F: (-2.01m, 2.01m), limbs within +-2^29
    fq2_sub(R, s2, acc.y);
    fq2_sqr(pp_, P);                           // 4.02^2
    fq2_sqr(rr_, R);
    if (__builtin_expect(fq2_is_zero_mod(pp_), 0)) {
        if (fq2_is_zero_mod(rr_)) {            // same point
            if (INLINE_SLOW) g2_dbl_affine_impl(acc, p.x, y2s);
            else { G2Xyzz d; const Fq2 px = p.x, py = y2s; g2_dbl_affine(d, px, py); acc = d; }     // (copies: the caller's values do not escape into the call)
        } else {
            g2_set_inf(acc);                   // opposite points
        }
        return;
    }
    fq2_mul(ppp, P, pp_);                      // 4.02 * 4
    fq2_mul(q, acc.x, pp_);                    // 4 * 4
    g2_add_tail(x3, y3, rr_, ppp, q, R, acc.y);
    fq2_mul(zz3, acc.zz, pp_);                 // 4 * 4
    fq2_mul(zzz3, acc.zzz, ppp);               // 4 * 2.02
    acc.x = x3; acc.y = y3; acc.zz = zz3; acc.zzz = zzz3;
}

// r = a + b, both stored-form XYZZ.   add-2008-s: 12 Fq2 products + 2 squarings
template <bool INLINE_SLOW = false>
KZG_HD void g2_add(G2Xyzz& r, const G2Xyzz& a, const G2Xyzz& b) {
    if (a.inf) { r = b; return; }
    if (b.inf) { r = a; return; }
    Fq2 u1, u2, s1, s2, P, R, pp_, rr_, ppp, q, t, x3, y3, zz3, zzz3;
    fq2_mul(u1, a.x, b.zz);                    // 4 * 4
    fq2_mul(u2, b.x, a.zz);
    fq2_mul(s1, a.y, b.zzz);
    fq2_mul(s2, b.y, a.zzz);
    fq2_sub(P, u2, u1);                        // class O - class O: |.| < 1.01m
    fq2_sub(R, s2, s1);
    fq2_sqr(pp_, P);
    fq2_sqr(rr_, R);
    if (__builtin_expect(fq2_is_zero_mod(pp_), 0)) {
        if (fq2_is_zero_mod(rr_)) {
            if (INLINE_SLOW) g2_dbl_impl(r, a);
            else { G2Xyzz d; const G2Xyzz ac = a; g2_dbl(d, ac); r = d; }
        } else {
            g2_set_inf(r);
        }
        return;
    }
    fq2_mul(ppp, P, pp_);                      // 2.02 * 4
    fq2_mul(q, u1, pp_);                       // 2.02 * 4
    g2_add_tail(x3, y3, rr_, ppp, q, R, s1);
    fq2_mul(t, a.zz, b.zz);                    // 4 * 4
    fq2_mul(zz3, t, pp_);                      // 2.02 * 4
    fq2_mul(t, a.zzz, b.zzz);
    fq2_mul(zzz3, t, ppp);
    r.x = x3; r.y = y3; r.zz = zz3; r.zzz = zzz3; r.inf = false;
}
KZG_HD_NOINLINE void g2_add_call(G2Xyzz& r, const G2Xyzz& a, const G2Xyzz& b) { g2_add<false>(r, a, b); }
// acc += v through the out-of-line addition, on copies: acc and v themselves do not escape into the call and stay in registers
KZG_HD void g2_add_into(G2Xyzz& acc, const G2Xyzz& v) {
    const G2Xyzz a = acc, b = v;
    G2Xyzz r;
    g2_add_call(r, a, b);
    acc = r;
}

// the twist constant 3 / (9 + u), class F
KZG_HD void g2_twist_b(Fq2& b) {
    const uint32_t bw[16] = {0x77b802a8u, 0x3bf938e3u, 0x3633535du, 0x020b1b27u, 0x49755260u, 0x26b7edf0u, 0x4384a86du, 0x2514c632u,
                             0xd1dcff67u, 0x38e7ecccu, 0x93ce0d3eu, 0x65f0b37du, 0x22ac00aau, 0xd749d0ddu, 0x4a688d4du, 0x0141b9ceu};   // wire form
    fq2_from_wire(b, bw);
}
// y^2 == x^3 + 3 / (9 + u) for affine coordinates in class F
KZG_HD bool g2_on_twist(const Fq2& x, const Fq2& y) {
    Fq2 b, yy, xx, xxx, d;
    g2_twist_b(b);
    fq2_sqr(yy, y);                            // 4 * 4
    fq2_sqr(xx, x);
    fq2_mul(xxx, xx, x);                       // 4 * 4
    fq2_sub(d, yy, xxx); fq2_sub(d, d, b);     // (-4.01m, 3.01m)
    fq2_reduce(d);
    return fq2_is_zero_mod(d);
}
// the generator of G2, wire form (x.c0 | x.c1 | y.c0 | y.c1)
KZG_HD void g2_generator_wire(uint32_t w[32]) {
    const uint32_t g[32] = {0x02bc2026u, 0x8e83b5d1u, 0x497b0172u, 0xdceb1935u, 0x97811adfu, 0xfbb82647u, 0xaf96503bu, 0x19573841u,
                            0xa84c6140u, 0xafb4737du, 0x5802d8c4u, 0x6043dd5au, 0x52a02f86u, 0x09e950fcu, 0x3aea7b6bu, 0x14fef083u,
                            0x886be9f6u, 0x619dfa9du, 0xf59e9b78u, 0xfe7fd297u, 0x231b7dfeu, 0xff9e1a62u, 0xae9e4206u, 0x28fd7eebu,
                            0xc71856eeu, 0x64095b56u, 0x327d3cbbu, 0xdc57f922u, 0x33351076u, 0x55f935beu, 0x93fd6482u, 0x0da4a0e6u};
#pragma unroll
    for (int j = 0; j < 32; ++j) w[j] = g[j];
}

// stored-form XYZZ -> affine coordinates in class F (one Fq2 inversion: x = X ZZZ / (ZZ ZZZ) * ..., taken as X / ZZ and Y / ZZZ
// with the single inverse of ZZ ZZZ).  v must not be the identity.
KZG_HD void g2_to_affine(Fq2& x, Fq2& y, const G2Xyzz& v) {
    Fq2 d, di, izz, izzz;
    fq2_mul(d, v.zz, v.zzz);                   // 4 * 4
    fq2_inv(di, d);
    fq2_mul(izz, di, v.zzz);                   // 1 / ZZ
    fq2_mul(izzz, di, v.zz);                   // 1 / ZZZ
    fq2_mul(x, v.x, izz);
    fq2_mul(y, v.y, izzz);
}

// ---------------------------------------------------------------------------------------------
// Memory formats
// ---------------------------------------------------------------------------------------------
// Device-resident affine point: 32 u32 = x.c0[8] | x.c1[8] | y.c0[8] | y.c1[8], canonical residues of the INTERNAL Montgomery form
// (a * 2^261 mod p), 128 B, read as eight 128-bit loads.  Identity = all zero.
KZG_HD bool g2_affine_load(G2Affine& p, const uint4* __restrict__ src) {
    uint4 q[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] = src[k];
    uint32_t w[32];
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        w[4 * k] = q[k].x; w[4 * k + 1] = q[k].y; w[4 * k + 2] = q[k].z; w[4 * k + 3] = q[k].w;
        any |= q[k].x | q[k].y | q[k].z | q[k].w;
    }
    fq2_unpack(p.x, w);
    fq2_unpack(p.y, w + 16);
    return any != 0;       // false = identity
}

// XYZZ in global memory: 72 int32 limbs, struct-of-arrays: limb k of element i at base[k * stride + i].
KZG_HD void g2_store(int32_t* __restrict__ base, size_t stride, size_t i, const G2Xyzz& v) {
    const Fq* c[8] = {&v.x.c0, &v.x.c1, &v.y.c0, &v.y.c1, &v.zz.c0, &v.zz.c1, &v.zzz.c0, &v.zzz.c1};
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int j = 0; j < NL; ++j) base[(size_t)(q * NL + j) * stride + i] = v.inf ? 0 : c[q]->l[j];
}
KZG_HD void g2_load(G2Xyzz& v, const int32_t* __restrict__ base, size_t stride, size_t i) {
    Fq* c[8] = {&v.x.c0, &v.x.c1, &v.y.c0, &v.y.c1, &v.zz.c0, &v.zz.c1, &v.zzz.c0, &v.zzz.c1};
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int j = 0; j < NL; ++j) c[q]->l[j] = base[(size_t)(q * NL + j) * stride + i];
    v.inf = fq2_is_literal_zero(v.zz);
}

// wire affine (32 u32, radix 2^256) -> device affine format; *on_twist: the point is the identity (all zero) or satisfies the equation
KZG_HD void g2_affine_wire_to_device(uint32_t out[32], const uint32_t in[32], bool* on_twist) {
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) any |= in[j];
    Fq2 x, y;
    fq2_from_wire(x, in);
    fq2_from_wire(y, in + 16);
    if (on_twist) *on_twist = any == 0 || g2_on_twist(x, y);
    fq2_pack_canonical(out, x);
    fq2_pack_canonical(out + 16, y);
}
// device affine format -> wire affine
KZG_HD void g2_affine_device_to_wire(uint32_t out[32], const uint32_t in[32]) {
    Fq2 x, y;
    fq2_unpack(x, in);
    fq2_unpack(y, in + 16);
    fq2_to_wire(out, x);
    fq2_to_wire(out + 16, y);
}
// stored-form XYZZ -> 64 u32 wire words X | Y | ZZ | ZZZ (radix 2^256, canonical); identity = zeros
KZG_HD void g2_to_wire(uint32_t out[64], const G2Xyzz& v) {
    if (v.inf) {
#pragma unroll
        for (int j = 0; j < 64; ++j) out[j] = 0;
        return;
    }
    fq2_to_wire(out, v.x);
    fq2_to_wire(out + 16, v.y);
    fq2_to_wire(out + 32, v.zz);
    fq2_to_wire(out + 48, v.zzz);
}

#if defined(__HIPCC__)
// a stored-form XYZZ value from another lane of the wave: lane + src_lane (down) or lane src_lane (g2msm.hip, g2batch.hip)
__device__ __forceinline__ void g2_shfl(G2Xyzz& r, const G2Xyzz& v, int src_lane, bool down) {
    const Fq* s[8] = {&v.x.c0, &v.x.c1, &v.y.c0, &v.y.c1, &v.zz.c0, &v.zz.c1, &v.zzz.c0, &v.zzz.c1};
    Fq* d[8] = {&r.x.c0, &r.x.c1, &r.y.c0, &r.y.c1, &r.zz.c0, &r.zz.c1, &r.zzz.c0, &r.zzz.c1};
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int j = 0; j < NL; ++j) d[q]->l[j] = down ? __shfl_down(s[q]->l[j], src_lane, 64) : __shfl(s[q]->l[j], src_lane, 64);
    r.inf = (down ? __shfl_down((int)v.inf, src_lane, 64) : __shfl((int)v.inf, src_lane, 64)) != 0;
}
#endif

}  // namespace kzg
