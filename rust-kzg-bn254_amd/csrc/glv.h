// glv.h — GLV scalar multiplication on BN254 G1 (lifted from g1fft.hip so that multiproof.hip shares it; the constants are per
// translation unit).  Used by the G1 FFT stages (g1fft.hip) and the FK20 linear combinations (multiproof.hip).
#pragma once
#include "curve.h"

namespace kzg {

// ---- GLV: k P = k1 P + k2 phi(P), phi(x, y) = (beta x, y) = [lambda] P on BN254 G1, |k1|, |k2| < 2^127 ---------------------------
// beta, lambda: the cube roots of unity of Fq / Fr with phi(G) = [lambda] G (checked with big integers: tools note in DESIGN.md 9);
// lattice basis of {(x, y): x + y lambda = 0 mod r} from the extended Euclid on (r, lambda):
//   (a1, b1) = (9931322734385697763, -147946756881789319000765030803803410728), (a2, b2) = (147946756881789319010696353538189108491, a1),
// a1 b2 - a2 b1 = r.  c1 = floor(k g1 / 2^256), c2 = floor(k g2 / 2^256) with g1 = round(2^256 b2 / r), g2 = round(2^256 (-b1) / r);
// k1 = k - c1 a1 - c2 a2, k2 = c1 |b1| - c2 b2.  The chains below read exactly 127 bits of each half.  With e1 = r |g1 - 2^256 b2 / r| / 2^256
// = 0.0818 and e2 likewise = 0.0665 (the rounding of g1, g2 scaled by k / 2^256 < r / 2^256), every canonical k has
//   |k2| <= (1 + e1) |b1| + e2 b2 = 0.94064746 2^127   (reached: k = 0x30644e1a4d7a33b8b20680a578b2ce9067544f5b7d240c6cd2a77771c2cfd9d4),
//   |k1| <= (1 + e1) a1 + (1 + e2) a2 = 0.92741129 2^127   (largest met: 0.86955288 2^127, a2 almost exactly),
// i.e. 6 % of headroom: one word less in g1 or a constant off by one puts a half over 2^127.  Signs: g1 is rounded down and g2 up, so
// k1 > -e2 a2 = -0.058 2^127 (> -2^123.9), and k2 <= 0 on every scalar of the tests (a positive k2 is at most b2 < 2^64); a decomposed
// scalar therefore never has a positive second half or a large negative first one.  Callers that pass halves of their own may use both
// signs of both.
// Derived from the constants below and checked by tests/test_glv_host.py; the device results by tests/test_gpu_glv.py.
// Little-endian 32-bit words.
static __device__ const uint32_t GLV_G1[3] = {0xc7e0b3d7u, 0xd91d232eu, 0x00000002u};
static __device__ const uint32_t GLV_G2[5] = {0x391eb18eu, 0x7a7bd9d4u, 0xa773d2cfu, 0x4ccef014u, 0x00000002u};
static __device__ const uint32_t GLV_A1[2] = {0x94d213e3u, 0x89d32568u};                                   // = b2
static __device__ const uint32_t GLV_B1M[4] = {0x7d4f1128u, 0x8211bbebu, 0xeeb859fcu, 0x6f4d8248u};        // -b1
static __device__ const uint32_t GLV_A2[4] = {0x1221250bu, 0x0be4e154u, 0xeeb859fdu, 0x6f4d8248u};
static __device__ const uint32_t GLV_BETA[8] = {0x77fffffeu, 0x57634731u, 0xacdb5c4fu, 0xd4f263f1u, 0xa0d48bacu, 0x59e26bceu, 0u, 0u};   // plain integer

// out[0 .. na+nb) = a * b (schoolbook, 32-bit words)
template <int NA, int NB>
__device__ __forceinline__ void glv_mul_words(uint32_t* out, const uint32_t* a, const uint32_t* b) {
#pragma unroll
    for (int i = 0; i < NA + NB; ++i) out[i] = 0;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const uint64_t t = (uint64_t)a[i] * b[j] + out[i + j] + carry;
            out[i + j] = (uint32_t)t;
            carry = t >> 32;
        }
        out[i + NB] = (uint32_t)carry;
    }
}
// 256-bit two's complement helpers
__device__ __forceinline__ void glv_sub8(uint32_t* r, const uint32_t* a, const uint32_t* b, int nb) {   // r = a - b (b has nb <= 8 words)
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t bi = i < nb ? b[i] : 0u;
        const uint64_t t = (uint64_t)a[i] - bi - borrow;
        r[i] = (uint32_t)t;
        borrow = (t >> 32) & 1u;
    }
}
__device__ __forceinline__ uint32_t glv_abs8(uint32_t* v) {                                             // v = |v|, returns the sign
    const uint32_t neg = v[7] >> 31;
    if (neg) {
        uint64_t carry = 1;
#pragma unroll
        for (int i = 0; i < 8; ++i) { const uint64_t t = (uint64_t)(~v[i]) + carry; v[i] = (uint32_t)t; carry = t >> 32; }
    }
    return neg;
}
// k (canonical, < r) -> kk[0..3] = |k1|, kk[4..7] = |k2|, their signs in bit 31 of kk[3] / kk[7]
__device__ __forceinline__ void glv_decompose(uint32_t kk[8], const uint32_t k[8]) {
    uint32_t p1[11], p2[13];
    glv_mul_words<8, 3>(p1, k, GLV_G1);
    glv_mul_words<8, 5>(p2, k, GLV_G2);
    const uint32_t c1[2] = {p1[8], p1[9]};                          // < 2^64  (p1[10] = 0: k g1 < 2^320)
    const uint32_t c2[4] = {p2[8], p2[9], p2[10], p2[11]};          // < 2^128 (p2[12] = 0)
    uint32_t t1[4], t2[8], t3[6], t4[6];
    glv_mul_words<2, 2>(t1, c1, GLV_A1);
    glv_mul_words<4, 4>(t2, c2, GLV_A2);
    glv_mul_words<2, 4>(t3, c1, GLV_B1M);
    glv_mul_words<4, 2>(t4, c2, GLV_A1);
    uint32_t k1[8], k2[8], z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    glv_sub8(k1, k, t1, 4);
    glv_sub8(k1, k1, t2, 8);
    uint32_t t3w[8] = {t3[0], t3[1], t3[2], t3[3], t3[4], t3[5], 0, 0};
    (void)z;
    glv_sub8(k2, t3w, t4, 6);
    const uint32_t s1 = glv_abs8(k1), s2 = glv_abs8(k2);
#pragma unroll
    for (int i = 0; i < 4; ++i) { kk[i] = k1[i]; kk[4 + i] = k2[i]; }
    kk[3] |= s1 << 31;
    kk[7] |= s2 << 31;
}

// r = [k] * p with k given as its GLV halves (glv_decompose): 127 doublings, each followed by ONE addition of +-P, +-phi(P) or their
// sum selected per lane (a wave executes the addition whenever any of its lanes has a bit set, i.e. always: the plain
// double-and-add paid 254 doublings AND 254 additions per wave)
__device__ __forceinline__ void xyzz_scalar_mul(Xyzz& r, const Xyzz& p, const uint32_t kk[8]) {
    if (p.inf) { xyzz_set_inf(r); return; }
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
    fe_mul(bx, p.x, beta);
    fe_cneg(y1, p.y, s1); fe_norm(y1);                             // stored form: the first addition to the identity returns P1 / P2 / S as it is
    fe_cneg(y2, p.y, s2); fe_norm(y2);
    Xyzz P1 = p, P2 = p, S;
    P1.y = y1;
    P2.x = bx; P2.y = y2;
    xyzz_add<true>(S, P1, P2);
    Xyzz acc;
    xyzz_set_inf(acc);
#pragma unroll 1
    for (int i = 126; i >= 0; --i) {
        Xyzz t;
        xyzz_dbl_impl(t, acc);
        acc = t;
        const uint32_t b1 = (kk[i >> 5] >> (i & 31)) & 1u, b2 = (kk[4 + (i >> 5)] >> (i & 31)) & 1u;
        Xyzz op;
        const bool both = b1 & b2;
        fe_select(op.x, both, S.x, b1 ? P1.x : P2.x);
        fe_select(op.y, both, S.y, b1 ? P1.y : P2.y);
        fe_select(op.zz, both, S.zz, p.zz);
        fe_select(op.zzz, both, S.zzz, p.zzz);
        op.inf = both ? S.inf : !(b1 | b2);
        xyzz_add<true>(t, acc, op);
        acc = t;
    }
    r = acc;
}

// [s] P with s a wire Fr scalar and P a device-format affine point (identity: zeros)
__device__ __forceinline__ void glv_term(Xyzz& r, const uint4* __restrict__ scalar, const uint4* __restrict__ point) {
    Affine p;
    if (!affine_load(p, point)) { xyzz_set_inf(r); return; }
    const uint4 lo = scalar[0], hi = scalar[1];
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t kc[8], kk[8];
    fe_wire_to_canonical_words<FrParams>(kc, w);
    glv_decompose(kk, kc);
    Xyzz base;
    xyzz_from_affine(base, p, 0);
    xyzz_scalar_mul(r, base, kk);
}

}  // namespace kzg
