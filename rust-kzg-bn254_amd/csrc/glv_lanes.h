// glv_lanes.h — the GLV scalar multiplication of glv.h on the lane-split point forms: one point on a PAIR of lanes (curve_pair.h) and on
// a QUAD of lanes (curve_quad.h).  Used by the G1 FFT stages (g1fft.hip, which says why and what each form measured); a header of
// its own so that the device conformance kernels (tests/devcheck) reach the same functions.
//
// Contract of both: k as its GLV halves (glv_decompose: 127-bit magnitudes, signs in bit 31 of kk[3] / kk[7]); every lane of a group
// holds the same k; every lane of the wave is active (the functions use __all and DPP moves); p in stored form or the identity.
#pragma once
#include "glv.h"
#include "curve_pair.h"
#include "curve_quad.h"

#if defined(__HIPCC__)
namespace kzg {

__device__ __forceinline__ void pair_dbl_any(HalfXyzz& r, const HalfXyzz& a, bool odd) {      // a may be the identity
    if (__all(a.inf)) { r = a; return; }
    HalfXyzz d;
    pair_dbl(d, a, odd);
    if (a.inf) r = a; else r = d;
}
// r = [k] p, k as its GLV halves (glv_decompose); every lane of a pair holds the same k
__device__ __forceinline__ void pair_scalar_mul(HalfXyzz& r, const HalfXyzz& p, const uint32_t kk[8], bool odd) {
    const uint32_t s1 = kk[3] >> 31, s2 = kk[7] >> 31;
    Fq beta, kin, bx, y1, y2;
    {
        uint32_t bw[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) bw[j] = GLV_BETA[j];
        fe_unpack(beta, bw);
#pragma unroll
        for (int j = 0; j < NL; ++j) kin.l[j] = (int32_t)FqParams::K_PLAIN_IN[j];
        fe_mul(beta, beta, kin);                                   // plain integer -> internal form
    }
    fe_mul(bx, p.u, beta);                                         // even lane: beta X
    fe_cneg(y1, p.u, s1); fe_norm(y1);                             // odd lane: +-Y
    fe_cneg(y2, p.u, s2); fe_norm(y2);
    HalfXyzz P1 = p, P2 = p, S;
    fe_select(P1.u, odd, y1, p.u);
    fe_select(P2.u, odd, y2, bx);
    pair_add(S, P1, P2, odd);
    HalfXyzz acc;
    half_set_inf(acc);
#pragma unroll 1
    for (int i = 126; i >= 0; --i) {
        HalfXyzz t;
        pair_dbl_any(t, acc, odd);
        acc = t;
        const uint32_t b1 = (kk[i >> 5] >> (i & 31)) & 1u, b2 = (kk[4 + (i >> 5)] >> (i & 31)) & 1u;
        HalfXyzz op;
        const bool both = b1 & b2;
        fe_select(op.u, both, S.u, b1 ? P1.u : P2.u);
        fe_select(op.v, both, S.v, p.v);
        op.inf = p.inf || (both ? S.inf : !(b1 | b2));
        pair_add(t, acc, op, odd);
        acc = t;
    }
    r = acc;
}

// TWO bits of each half per step on a quad (see the body): r = [k] p
__device__ __forceinline__ void quad_scalar_mul(QuadXyzz& r, const QuadXyzz& p, const uint32_t kk[8], uint32_t q) {
    const uint32_t s1 = kk[3] >> 31, s2 = kk[7] >> 31;
    Fq beta, kin, bx, y1, y2;
    {
        uint32_t bw[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) bw[j] = GLV_BETA[j];
        fe_unpack(beta, bw);
#pragma unroll
        for (int j = 0; j < NL; ++j) kin.l[j] = (int32_t)FqParams::K_PLAIN_IN[j];
        fe_mul(beta, beta, kin);                                   // plain integer -> internal form
    }
    fe_mul(bx, p.c, beta);                                         // lane 0: beta X
    fe_cneg(y1, p.c, s1); fe_norm(y1);                             // lane 1: +-Y
    fe_cneg(y2, p.c, s2); fe_norm(y2);
    QuadXyzz P1 = p, P2 = p;
    fe_select(P1.c, q == 1u, y1, p.c);
    fe_select(P2.c, q == 1u, y2, p.c);
    fe_select(P2.c, q == 0u, bx, P2.c);
    // TWO bits of each half per step: two doublings and ONE addition of T[a + 4 b] = a P1 + b P2, a, b < 4 (3 + 3 + 4 = 10 products deep per two
    // bits instead of 14).  On a quad a point is nine words per lane, so the fifteen table points of a lane stay in registers (135 VGPRs)
    // and the entry is picked with a v_cndmask tree (keeping them in an LDS column per lane instead measured the same time per stage: docs/history).
    // No entry is the identity unless p is (a + b lambda != 0 mod r for these a, b): one flag for all.
    QuadXyzz t, u;
    Fq T[16];                                                      // T[0] unused
    T[1] = P1.c; T[4] = P2.c;
    Fq p1x2, p1x3, p2x2, p2x3;
    quad_dbl_any(t, P1, q); p1x2 = t.c; T[2] = t.c;
    quad_add(u, t, P1, q); p1x3 = u.c; T[3] = u.c;
    quad_dbl_any(t, P2, q); p2x2 = t.c; T[8] = t.c;
    quad_add(u, t, P2, q); p2x3 = u.c; T[12] = u.c;
#pragma unroll
    for (int bb = 1; bb < 4; ++bb)
#pragma unroll
        for (int aa = 1; aa < 4; ++aa) {
            QuadXyzz x, y;
            x.c = aa == 1 ? P1.c : aa == 2 ? p1x2 : p1x3; x.inf = p.inf;
            y.c = bb == 1 ? P2.c : bb == 2 ? p2x2 : p2x3; y.inf = p.inf;
            quad_add(t, x, y, q);
            T[aa + 4 * bb] = t.c;
        }
    QuadXyzz acc;
    quad_set_inf(acc);
    // the two 127-bit halves as shift registers (a dynamically indexed kk[] would live in scratch memory): the window is the top two bits
    uint32_t h1[4] = {kk[0], kk[1], kk[2], kk[3] & 0x7FFFFFFFu}, h2[4] = {kk[4], kk[5], kk[6], kk[7] & 0x7FFFFFFFu};   // bit 127 is the sign
#pragma unroll 1
    for (int i = 63; i >= 0; --i) {                                // bits 2 i + 1, 2 i of both halves
        const uint32_t a = h1[3] >> 30, b = h2[3] >> 30;
#pragma unroll
        for (int j = 3; j > 0; --j) { h1[j] = (h1[j] << 2) | (h1[j - 1] >> 30); h2[j] = (h2[j] << 2) | (h2[j - 1] >> 30); }
        h1[0] <<= 2; h2[0] <<= 2;
        const uint32_t idx = a | (b << 2);
        QuadXyzz op;
        // 16-way select as a binary tree over the index bits (entry 0 never used as a point: op.inf covers it)
        Fq s8[8], s4[4], s2[2];
#pragma unroll
        for (int m = 0; m < 8; ++m) fe_select(s8[m], (idx & 1u) != 0, T[2 * m + 1], T[m == 0 ? 1 : 2 * m]);
#pragma unroll
        for (int m = 0; m < 4; ++m) fe_select(s4[m], (idx & 2u) != 0, s8[2 * m + 1], s8[2 * m]);
#pragma unroll
        for (int m = 0; m < 2; ++m) fe_select(s2[m], (idx & 4u) != 0, s4[2 * m + 1], s4[2 * m]);
        fe_select(op.c, (idx & 8u) != 0, s2[1], s2[0]);
        op.inf = p.inf || idx == 0u;
        quad_dbl_any(t, acc, q);
        quad_dbl_any(acc, t, q);
        quad_add(t, acc, op, q);
        acc = t;
    }
    r = acc;
}

}  // namespace kzg
#endif
