// g1fft.hip — `KZG::g1_ifft` (prover/src/kzg.rs:263-285): the inverse FFT whose DATA are G1 points and whose
// twiddles are Fr scalars,  L_i = n^-1 * sum_j w^(-ij) P_j  (natural order) — the Lagrange-basis SRS.
// Reference: `GeneralEvaluationDomain::<Fr>::new(n).ifft(&[G1Projective])` + n `into_affine()` inversions, recomputed on
// every `commit_eval_form` (kzg.rs:96-98).  The commit / proof path of this library never needs it
// (commit_eval_form == MSM(srs, IFFT(evals))); it is public API with its own bench
// (prover/benches/bench_g1_ifft.rs) and golden vector (prover/tests/test-files/lagrangeG1SRS.txt), and the library can keep
// its result on the device as an SRS of its own (kzg_srs_lagrange) so that eval-form commitments become one MSM.
//
// What bounds it on a GPU is DEPTH: every FFT stage multiplies points by full-width scalars, i.e. a chain of ~254 dependent
// doublings (~4 us each on a lone wave), and radix 2 has log2 n such stages.  Work is spent to cut the depth:
//   * small n (n * R <= 65536 lanes): Stockham stages of radix R = 2^k, k <= 5, each output as a DIRECT sum of its R inputs,
//       y[u + j N/R] = sum_j' [w^-(s p j' + (N/R) j j')] x[q + s (R p + j')],   u = q + s p,
//     one lane per (output, term): one scalar multiplication deep per stage plus a k-step shuffle tree, ceil(log2 n / 5) stages
//     instead of log2 n (n = 2048: 3 instead of 11), for (2^k - 1)/k times the multiplications;
//   * large n: radix-2 butterflies (A, B) -> (A + [w]B, A - [w]B), one multiplication per two outputs (work bound);
//   * the scaling by n^-1 is folded into the scalars of the last stage (no chain of its own);
//   * Jacobian -> affine by Montgomery's trick (one inversion per lane for 16 points) when there are many points.
#include "engine.h"
#include "curve_pair.h"
#include "curve_quad.h"
#include "fe_invert.h"
#include "g1_decode.h"   // g1_compress_point: the affine conversion's compressed output
#include "naf.h"
#include "glv.h"
#include "glv_lanes.h"
#include "host_curve.h"
#include "g1fft_plan.h"
#include "host_encode.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <tuple>
#include <mutex>
#include <vector>

namespace kzg {

__device__ __forceinline__ void tw_load(Fr& w, const NttTables& tb, uint32_t E) {
#pragma unroll
    for (int j = 0; j < NL; ++j) w.l[j] = tb.lo[(size_t)j * tb.lo_len + (E & (tb.lo_len - 1))];
    uint32_t eh = E >> tb.lo_bits;
    if (eh != 0) {
        Fr h;
#pragma unroll
        for (int j = 0; j < NL; ++j) h.l[j] = tb.hi[(size_t)j * tb.hi_len + eh];
        fe_mul(w, w, h);
    }
}

// k = entry e of a scalar table (k_g1fft_scalars): eight words
__device__ __forceinline__ void scal_load(uint32_t k[8], const uint4* __restrict__ scal, uint32_t e) {
    const uint4 lo = scal[2 * (size_t)e], hi = scal[2 * (size_t)e + 1];
    k[0] = lo.x; k[1] = lo.y; k[2] = lo.z; k[3] = lo.w; k[4] = hi.x; k[5] = hi.y; k[6] = hi.z; k[7] = hi.w;
}

// scal[e] = the GLV halves (glv_decompose) of the canonical integer of w^-e, or of w^-e / n (scaled != 0), e < n: the scalars of every stage
// (canon != 0: the canonical 256-bit integer itself, for the window-table stage)
__global__ void __launch_bounds__(256)
k_g1fft_scalars(uint4* __restrict__ scal, uint32_t n, int log_n, NttTables tb_inv, int scaled, int canon) {
    uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    Fr w;
    if (log_n > 0) tw_load(w, tb_inv, e); else fe_set_one(w);
    if (scaled) {
        Fr ninv;
#pragma unroll
        for (int j = 0; j < NL; ++j) ninv.l[j] = (int32_t)FrParams::NINV[log_n * NL + j];
        fe_mul(w, w, ninv);
    }
    Fr one_plain, c;
    fe_set_zero(one_plain);
    one_plain.l[0] = 1;
    fe_mul(c, w, one_plain);                       // internal Montgomery form -> plain integer
    fe_canon(c);
    uint32_t kc[8], k[8];
    fe_pack(kc, c);
    if (canon == 2) {                                // wire words (arkworks Montgomery form): the scalars of an MSM
        fe_to_wire(k, w);
    } else if (canon) {
#pragma unroll
        for (int j = 0; j < 8; ++j) k[j] = kc[j];
    } else {
        glv_decompose(k, kc);
    }
    scal[2 * (size_t)e] = make_uint4(k[0], k[1], k[2], k[3]);
    scal[2 * (size_t)e + 1] = make_uint4(k[4], k[5], k[6], k[7]);
}

// planes[i] = P[i] as XYZZ (natural order: the Stockham stages sort on the way)
__global__ void __launch_bounds__(256)
k_g1fft_load(const uint4* __restrict__ points, uint32_t n, int32_t* __restrict__ planes, int bitrev_log) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t j = bitrev_log > 0 ? (__brev(i) >> (32 - bitrev_log)) : i;
    Affine p;
    Xyzz v;
    if (affine_load(p, points + 4 * (size_t)j)) xyzz_from_affine(v, p, 0);
    else xyzz_set_inf(v);
    xyzz_store(planes, n, i, v);
}

// ---- small n: one Stockham stage of radix R = 2^K as direct sums, one lane per (output, term) ---------------------------
__global__ void __launch_bounds__(256)
k_g1fft_direct(const int32_t* __restrict__ x, int32_t* __restrict__ y, uint32_t n, int log_n, int K, int log_s,
               const uint4* __restrict__ scal /* n canonical scalars: w^-e, or w^-e / n in the last stage */, int last,
               size_t x_batch, size_t y_batch /* words between the plane sets of consecutive transforms of a batch (grid.y) */) {
    x += blockIdx.y * x_batch;
    y += blockIdx.y * y_batch;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const uint32_t R = 1u << K;
    const uint32_t o = t >> K, jp = t & (R - 1);                 // output element, term j'
    const bool active = o < n;
    Xyzz term;
    xyzz_set_inf(term);
    if (active) {
        const uint32_t nr = n >> K;                               // N / R
        const uint32_t u = o & (nr - 1), j = o >> (log_n - K);
        const uint32_t s = 1u << log_s;
        const uint32_t q = u & (s - 1), p = u >> log_s;
        const uint32_t e = (uint32_t)(((unsigned long long)p * jp << log_s) + (unsigned long long)nr * j * jp) & (n - 1);
        Xyzz v;
        xyzz_load(v, x, n, (size_t)q + ((size_t)(R * p + jp) << log_s));
        if (e == 0 && !last) {
            term = v;
        } else {
            uint32_t k[8];
            scal_load(k, scal, e);
            xyzz_scalar_mul(term, v, k);
        }
    }
    // sum of the R terms of an output: R consecutive lanes (R <= 32 < 64: a wave holds whole outputs)
#pragma unroll 1
    for (int d = 1; d < (int)R; d <<= 1) {
        Xyzz other, r;
        const Fq* sp[4] = {&term.x, &term.y, &term.zz, &term.zzz};
        Fq* tp[4] = {&other.x, &other.y, &other.zz, &other.zzz};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int l = 0; l < NL; ++l) tp[c]->l[l] = __shfl_down(sp[c]->l[l], d, 64);
        other.inf = __shfl_down((int)term.inf, d, 64) != 0;
        if ((lane & (2 * d - 1)) == 0) {
            xyzz_add<true>(r, term, other);
            term = r;
        }
    }
    if (active && jp == 0) xyzz_store(y, n, o, term);
}

// ---- large n: radix-2 decimation in time on bit-reversed input, one butterfly per thread, in place ------------------------
__global__ void __launch_bounds__(256)
k_g1fft_stage(int32_t* __restrict__ planes, uint32_t n, int log_n, int s, const uint4* __restrict__ scal, int last, size_t batch_stride) {
    planes += blockIdx.y * batch_stride;
    uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n / 2) return;
    const uint32_t half = 1u << (s - 1);
    const uint32_t j = b & (half - 1);
    const uint32_t i0 = ((b >> (s - 1)) << s) | j, i1 = i0 + half;
    Xyzz A, B, t;
    xyzz_load(A, planes, n, i0);
    xyzz_load(B, planes, n, i1);
    const uint32_t E = j << (log_n - s);                 // w_n^(-j n/m)
    if (last) {                                          // (A +- [w]B) / n = [1/n]A +- [w/n]B: both products in this stage
        uint32_t k0[8];
        scal_load(k0, scal, 0);
        Xyzz a2;
        xyzz_scalar_mul(a2, A, k0);
        A = a2;
    }
    if (E == 0 && !last) {
        t = B;
    } else {
        uint32_t k[8];
        scal_load(k, scal, E);
        xyzz_scalar_mul(t, B, k);
    }
    Xyzz r0, r1, tn = t;
    if (!tn.inf) { fe_neg(tn.y, t.y); fe_norm(tn.y); }
    xyzz_add<true>(r0, A, t);
    xyzz_add<true>(r1, A, tn);
    xyzz_store(planes, n, i0, r0);
    xyzz_store(planes, n, i1, r1);
}

// ---- the same two stage kernels on LANE PAIRS (curve_pair.h): one point per two lanes ----------------------------------------
// A stage is one scalar multiplication deep: 127 doublings + 127 additions one after the other.  On a pair of lanes a doubling costs
// 5 multiplications per lane instead of 9 and an addition 7 instead of 14, and the doubled number of waves fills the issue slots a
// lone wave per SIMD leaves empty: 1.45 -> ~0.8 ms per stage.  Same group elements (the affine results are bit-identical).
// pair_dbl_any and pair_scalar_mul: glv_lanes.h.
__global__ void __launch_bounds__(256)
k_g1fft_direct_pairs(const int32_t* __restrict__ x, int32_t* __restrict__ y, uint32_t n, int log_n, int K, int log_s,
                     const uint4* __restrict__ scal, int last, size_t x_batch, size_t y_batch) {
    x += blockIdx.y * x_batch;
    y += blockIdx.y * y_batch;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63, pair = t >> 1;
    const bool odd = (t & 1u) != 0;
    const uint32_t R = 1u << K;
    const uint32_t o = pair >> K, jp = pair & (R - 1);           // output element, term j'
    const bool active = o < n;
    HalfXyzz term;
    half_set_inf(term);
    uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool plain = true;                                            // the term is the input itself (scalar 1)
    if (active) {
        const uint32_t nr = n >> K;
        const uint32_t u = o & (nr - 1), j = o >> (log_n - K);
        const uint32_t q = u & ((1u << log_s) - 1), p = u >> log_s;
        const uint32_t e = (uint32_t)(((unsigned long long)p * jp << log_s) + (unsigned long long)nr * j * jp) & (n - 1);
        half_load(term, x, n, (size_t)q + ((size_t)(R * p + jp) << log_s), odd);
        if (!(e == 0 && !last)) {
            scal_load(k, scal, e);
            plain = false;
        }
    }
    if (!__all(plain)) {                                          // wave-uniform: the multiplication runs for the whole wave or not at all
        HalfXyzz m;
        pair_scalar_mul(m, term, k, odd);
        if (!plain) term = m;
    }
    // sum of the R terms of an output: R consecutive pairs (R <= 32: a wave holds whole outputs)
#pragma unroll 1
    for (int d = 1; d < (int)R; d <<= 1) {
        HalfXyzz other;
        half_shfl_down(other, term, 2 * d);
        if (((lane >> 1) & (2 * d - 1)) == 0) {
            HalfXyzz r;
            pair_add(r, term, other, odd);
            term = r;
        }
    }
    if (active && jp == 0) half_store(y, n, o, term, odd);
}

// ---- the direct stage on LANE QUADS (curve_quad.h; round 4) -------------------------------------------------------------------------
// One step of the GLV chain is a doubling and an addition one after the other: 5 + 7 products deep on a lane pair, 3 + 4 on a quad.  A stage
// that fits one wave per SIMD is pure latency, so the quad form takes 7 / 12 of the pair form's time (measured: 0.83 -> 0.60 ms; with two bits
// per step 3 + 3 + 4 per two bits); the products
// [k] x of all (output, term) slots go to a partial array and k_g1fft_sum_partials adds the R = 2^K terms of an output (a wave holds 16 quads,
// so the tree no longer fits the multiplying wave for R = 32).  quad_scalar_mul: glv_lanes.h.

// slot (o, j') of a direct stage of radix R = 2^K (the index rule of k_g1fft_direct_pairs): partial[o R + j'] = [w^-e (/ n)] x[input]
__global__ void __launch_bounds__(256)
k_g1fft_mul_quads(const int32_t* __restrict__ x, int32_t* __restrict__ partial, uint32_t n, int log_n, int K, int log_s,
                  const uint4* __restrict__ scal, int last) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, q = t & 3u, quad = t >> 2;
    const uint32_t R = 1u << K;
    const uint32_t o = quad >> K, jp = quad & (R - 1);
    const bool active = o < n;
    QuadXyzz term;
    quad_set_inf(term);
    uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool plain = true;                                            // the term is the input itself (scalar 1)
    if (active) {
        const uint32_t nr = n >> K;
        const uint32_t u = o & (nr - 1), j = o >> (log_n - K);
        const uint32_t qq = u & ((1u << log_s) - 1), p = u >> log_s;
        const uint32_t e = (uint32_t)(((unsigned long long)p * jp << log_s) + (unsigned long long)nr * j * jp) & (n - 1);
        quad_load(term, x, n, (size_t)qq + ((size_t)(R * p + jp) << log_s), q);
        if (!(e == 0 && !last)) {
            scal_load(k, scal, e);
            plain = false;
        }
    }
    if (!__all(plain)) {                                          // wave-uniform: the multiplication runs for the whole wave or not at all
        QuadXyzz m;
        quad_scalar_mul(m, term, k, q);
        if (!plain) term = m;
    }
    if (active) quad_store(partial, (size_t)n * R, (size_t)o * R + jp, term, q);
}

__global__ void __launch_bounds__(256)
k_g1fft_stage_pairs(int32_t* __restrict__ planes, uint32_t n, int log_n, int s, const uint4* __restrict__ scal, int last, size_t batch_stride) {
    planes += blockIdx.y * batch_stride;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, b = t >> 1;
    const bool odd = (t & 1u) != 0;
    const bool active = b < n / 2;                               // n / 2 >= 32 pairs here: whole waves are active or not, except the last one
    const uint32_t half = 1u << (s - 1);
    const uint32_t j = b & (half - 1);
    const uint32_t i0 = active ? (((b >> (s - 1)) << s) | j) : 0, i1 = i0 + half;
    HalfXyzz A, B, tB;
    half_load(A, planes, n, i0, odd);
    half_load(B, planes, n, i1, odd);
    if (!active) { half_set_inf(A); half_set_inf(B); }
    const uint32_t E = j << (log_n - s);
    if (last) {                                                   // (A +- [w]B) / n = [1/n]A +- [w/n]B
        uint32_t k0[8];
        scal_load(k0, scal, 0);
        HalfXyzz a2;
        pair_scalar_mul(a2, A, k0, odd);
        A = a2;
    }
    const bool plain = E == 0 && !last;
    tB = B;
    if (!__all(plain)) {
        uint32_t k[8];
        scal_load(k, scal, E);
        HalfXyzz m;
        pair_scalar_mul(m, B, k, odd);
        if (!plain) tB = m;
    }
    HalfXyzz r0, r1, tn = tB;
    {
        Fq ny;
        fe_neg(ny, tB.u); fe_norm(ny);
        fe_select(tn.u, odd && !tB.inf, ny, tB.u);                // -[w]B: the odd lane's Y changes sign
    }
    pair_add(r0, A, tB, odd);
    pair_add(r1, A, tn, odd);
    if (active) {
        half_store(planes, n, i0, r0, odd);
        half_store(planes, n, i1, r1, odd);
    }
}

// ---- the FIRST stage through the SRS window tables --------------------------------------------------------------------------------
// The inputs of the first stage are SRS points, and the SRS carries window tables T_w[i] = 2^(c w) P_i for its MSMs.  So a term
// [k] P_i = sum_w d_w(k) T_w[i] with the signed c-bit digits of k: W small multiplications of c double-and-add steps (the addend is an
// AFFINE table point: pair_madd) instead of one 127-step GLV chain -- c x (5 + 5) multiplications deep instead of 127 x (5 + 7) -- and
// a tree over the R W terms of an output.  One PAIR of lanes per (output, term, window); a wave holds 32 (term, window) slots of one
// output and leaves their sum; k_g1fft_sum_partials adds the waves of an output.  Same group elements.
__global__ void __launch_bounds__(256)
k_g1fft_first_tables(const uint4* __restrict__ tables, uint32_t table_stride, int c, int W, uint32_t n, int log_n, int K,
                     const uint4* __restrict__ scal_canon, uint32_t waves_per_out, int32_t* __restrict__ partial) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63, pair = lane >> 1;
    const bool odd = (t & 1u) != 0;
    const uint32_t gw = t >> 6;
    const uint32_t o = gw / waves_per_out, wv = gw - o * waves_per_out;
    if (o >= n) return;                                           // wave-uniform
    const uint32_t R = 1u << K, nr = n >> K;
    const uint32_t tt = wv * 32 + pair;
    const bool valid = tt < R * (uint32_t)W;
    const uint32_t jp = valid ? tt / (uint32_t)W : 0, w = valid ? tt - jp * (uint32_t)W : 0;
    const uint32_t u = o & (nr - 1), j = o >> (log_n - K);
    const uint32_t e = (uint32_t)((unsigned long long)nr * j * jp) & (n - 1);
    const uint32_t i = u + nr * jp;                               // first stage: stride s = N / R, p = 0
    // signed c-bit digit number w of the canonical scalar (the MSM's digit rule: k_msm_digits)
    uint32_t mag = 0, neg = 0;
    {
        uint32_t k[8];
        scal_load(k, scal_canon, e);
        const uint32_t mask = (1u << c) - 1u, half = 1u << (c - 1);
        uint32_t carry = 0;
        for (uint32_t ww = 0; ww <= w; ++ww) {
            const uint32_t raw = (k[0] & mask) + carry;
#pragma unroll
            for (int q = 0; q < 7; ++q) k[q] = (k[q] >> c) | (k[q + 1] << (32 - c));
            k[7] >>= c;
            neg = raw > half;
            mag = neg ? (1u << c) - raw : raw;
            carry = neg;
        }
        if (!valid) mag = 0;
    }
    const uint4* src = tables + 4 * ((size_t)w * table_stride + i) + (odd ? 2 : 0);
    const uint4 q0 = src[0], q1 = src[1];                         // even lane: x, odd lane: y
    const uint32_t w32[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    int any = (q0.x | q0.y | q0.z | q0.w | q1.x | q1.y | q1.z | q1.w) != 0 ? 1 : 0;
    any |= pair_swap(any);
    if (!any) mag = 0;                                            // identity table point
    Fq cpt;
    fe_unpack(cpt, w32);
    HalfXyzz acc;
    half_set_inf(acc);
#pragma unroll 1
    for (int b = c - 1; b >= 0; --b) {
        HalfXyzz r;
        pair_dbl_any(r, acc, odd);
        acc = r;
        if ((mag >> b) & 1u) {                                    // pair-uniform
            pair_madd(r, acc, cpt, neg, odd);
            acc = r;
        }
    }
#pragma unroll 1
    for (int d = 1; d < 32; d <<= 1) {                            // sum of the wave's 32 slots
        HalfXyzz other;
        half_shfl_down(other, acc, 2 * d);
        if ((pair & (2 * d - 1)) == 0) {
            HalfXyzz r;
            pair_add(r, acc, other, odd);
            acc = r;
        }
    }
    if (pair == 0) half_store(partial, (size_t)n * waves_per_out, (size_t)o * waves_per_out + wv, acc, odd);
}
// ---- the WHOLE transform of 64 .. 256 points through the per-bit SRS tables ----------------------------------------------------------
// An SRS of >= 2^15 points carries Bit_p[j] = 2^p P_j for every bit position p (srs.hip srs_build_bit_tables, the NAF mode of its
// MSMs).  With the scalars in plain non-adjacent form (digits +-1, ~85 per scalar) a term [k] P_j is a SUM OF TABLE POINTS,
// sum_t +-Bit_(p_t)[j], and an output L_o = sum_j [w^(-o j) / n] P_j is n x 85 signed table points: no doubling, no scalar
// multiplication, no stages -- mixed additions at the chip's throughput (n^2 x 85: 5.6 M for n = 256) and one tree.  The n distinct
// scalars are recoded once per size (k_g1fft_naf2); one PAIR of lanes per (output, term, slice of the digit list) adds its digits
// (pair_madd, 5 multiplications per lane); a wave holds 32 slots of one output and leaves their sum; k_g1fft_sum_partials adds the
// <= 32 waves of an output.  Same group elements as the staged transform.
constexpr uint32_t NAF2_MAX = 128;                       // digit slots per scalar (width-4 NAF of a scalar < 2^254: at most 254 / 4 + 1 = 64)
// The odd multiples 3, 5, 7 of Bit_p[j] as XYZZ planes: k_g1fft_to_affine turns them into the tables.  3 x 255 x t3_points points (100 MB at
// 2 048), once per SRS (kzg_srs::d_t3, ::t3_n).
__global__ void __launch_bounds__(256)
k_g1fft_t3_planes(const uint4* __restrict__ bits, uint32_t stride, uint32_t t3_points, uint32_t total, int32_t* __restrict__ planes) {
    // slot t = ((key - 1) 255 + p) t3_points + j, key = 1, 2, 3: (2 key + 1) Bit_p[j] = Bit_p + Bit_(p+1) | Bit_p + Bit_(p+2) | Bit_(p+3) - Bit_p
    // (round 4: width-4 digits +-1, +-3, +-5, +-7).  A slot whose second plane would be beyond bit 254 stays the identity: no scalar
    // below the group order has such a digit (5 2^252 and 7 2^251 exceed it even with every lower digit negative).
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint32_t row = t / t3_points, j = t - row * t3_points;          // t3_points <= stride: every read stays inside its bit plane
    const uint32_t key = row / 255u + 1u, p = row - (key - 1u) * 255u;
    Xyzz v;
    xyzz_set_inf(v);
    if (p + key <= 254u) {
        Affine a, b;
        const bool ha = affine_load(a, bits + 4 * ((size_t)p * stride + j));
        const bool hb = affine_load(b, bits + 4 * ((size_t)(p + key) * stride + j));
        if (ha && hb) {
            if (key < 3u) { xyzz_from_affine(v, a, 0); xyzz_madd<true>(v, b, 0); }
            else { xyzz_from_affine(v, b, 0); xyzz_madd<true>(v, a, 1); }
        }
    }
    xyzz_store(planes, total, t, v);
}
__global__ void __launch_bounds__(64)
k_g1fft_naf2(const uint4* __restrict__ scal_canon, uint32_t n, uint16_t* __restrict__ list, uint32_t* __restrict__ cnt) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    uint32_t k[8];
    scal_load(k, scal_canon, e);
    uint32_t m = 0;
    // width-4 NAF (round 4; width 3 before): digits +-1, +-3, +-5, +-7 (key = 0 .. 3), ~51 per scalar instead of ~64; a digit with key > 0
    // reads the table of that odd multiple.  Entry: position (8 bits) | key << 8 | sign << 15
    naf_for_digits(k, 4, [&](uint32_t pos, uint32_t key, uint32_t neg) { if (m < NAF2_MAX) list[(size_t)e * NAF2_MAX + m] = (uint16_t)(pos | (key << 8) | (neg << 15)); ++m; });
    cnt[e] = m < NAF2_MAX ? m : NAF2_MAX;
}
// K < log n: the same kernel as the FIRST STAGE of a staged transform of radix R = 2^K (the index rule of k_g1fft_first_tables: output o
// sums the R inputs u + (n / R) j' with the scalars w^-(n / R . j . j'), u = o mod n / R, j = o / (n / R)); K = log n is the whole transform.
__global__ void __launch_bounds__(256)
k_g1fft_bits(const uint4* __restrict__ bits, uint32_t stride, const uint4* __restrict__ bits3 /* 3 Bit_p[i], i < t3_points, that many points apart */,
             uint32_t t3_points, uint32_t n, int log_n, int K, const uint16_t* __restrict__ list, const uint32_t* __restrict__ cnt,
             uint32_t Q, uint32_t waves_per_out, int32_t* __restrict__ partial) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63, pair = lane >> 1;
    const bool odd = (t & 1u) != 0;
    const uint32_t gw = t >> 6;
    const uint32_t o = gw / waves_per_out, wv = gw - o * waves_per_out;
    if (o >= n) return;                                           // wave-uniform
    const uint32_t slot = wv * 32 + pair;                         // < R Q (the host makes R Q a multiple of 32)
    const uint32_t jp = slot / Q, q = slot - jp * Q;
    const uint32_t nr = n >> K, u = o & (nr - 1), jo = o >> (log_n - K);
    const uint32_t j = u + nr * jp;                               // the input point
    const uint32_t e = (uint32_t)((unsigned long long)nr * jo * jp) & (n - 1);
    const uint16_t* L = list + (size_t)e * NAF2_MAX;
    const uint32_t c = cnt[e];
    HalfXyzz acc;
    half_set_inf(acc);
    // digit m of the list: the table point Bit_pos[j], even lane x, odd lane y; one point in flight ahead of the addition
    auto fetch = [&](uint32_t m, uint4& a, uint4& b, uint32_t& neg) {
        const uint32_t d = L[m < c ? m : (c ? c - 1 : 0)];
        neg = d >> 15;
        const uint32_t pos = d & 0xFFu, key = (d >> 8) & 3u;
        const uint4* src = (key ? bits3 + 4 * ((size_t)((key - 1u) * 255u + pos) * t3_points + j) : bits + 4 * ((size_t)pos * stride + j)) + (odd ? 2 : 0);
        a = src[0]; b = src[1];
    };
    uint4 a0, b0; uint32_t neg0 = 0;
    if (c) fetch(q, a0, b0, neg0);
#pragma unroll 1
    for (uint32_t m = q; m < c; m += Q) {                         // pair-uniform trip count
        const uint32_t w32[8] = {a0.x, a0.y, a0.z, a0.w, b0.x, b0.y, b0.z, b0.w};
        const uint32_t neg = neg0;
        int any = (a0.x | a0.y | a0.z | a0.w | b0.x | b0.y | b0.z | b0.w) != 0 ? 1 : 0;
        any |= pair_swap(any);
        fetch(m + Q, a0, b0, neg0);
        if (!any) continue;                                       // identity SRS point
        Fq cpt;
        fe_unpack(cpt, w32);
        HalfXyzz r;
        pair_madd(r, acc, cpt, neg, odd);
        acc = r;
    }
#pragma unroll 1
    for (int d = 1; d < 32; d <<= 1) {                            // sum of the wave's 32 slots
        HalfXyzz other;
        half_shfl_down(other, acc, 2 * d);
        if ((pair & (2 * d - 1)) == 0) {
            HalfXyzz r;
            pair_add(r, acc, other, odd);
            acc = r;
        }
    }
    if (pair == 0) half_store(partial, (size_t)n * waves_per_out, (size_t)o * waves_per_out + wv, acc, odd);
}
// y[o] = sum of the waves_per_out (<= 32) partial sums of output o: one wave per output
__global__ void __launch_bounds__(256)
k_g1fft_sum_partials(const int32_t* __restrict__ partial, uint32_t waves_per_out, uint32_t n, int32_t* __restrict__ y) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63, pair = lane >> 1;
    const bool odd = (t & 1u) != 0;
    const uint32_t o = t >> 6;
    if (o >= n) return;
    HalfXyzz acc;
    if (pair < waves_per_out) half_load(acc, partial, (size_t)n * waves_per_out, (size_t)o * waves_per_out + pair, odd);
    else half_set_inf(acc);
#pragma unroll 1
    for (int d = 1; d < 32; d <<= 1) {
        HalfXyzz other;
        half_shfl_down(other, acc, 2 * d);
        if ((pair & (2 * d - 1)) == 0) {
            HalfXyzz r;
            pair_add(r, acc, other, odd);
            acc = r;
        }
    }
    if (pair == 0) half_store(y, n, o, acc, odd);
}

// ---- XYZZ -> affine ------------------------------------------------------------------------------------------------------
// BYTES: the point leaves as its 32 gnark-compressed bytes (g1_decode.h g1_compress_point; the identity 0x40 || zeros, no flag beside it),
// two uint4 per point instead of four; `wire` is then unused
template <bool BYTES>
__device__ __forceinline__ void affine_emit(uint4* __restrict__ out, size_t i, const Xyzz& r, const Fq& inv_zz_zzz /* 1 / (ZZ ZZZ) */, bool wire) {
    if (BYTES) {
        uint32_t o[8];
        Fq t, x, y;
        fe_set_zero(x);
        fe_set_zero(y);
        if (!r.inf) {
            fe_mul(t, inv_zz_zzz, r.zzz);          // 1 / ZZ
            fe_mul(x, r.x, t);
            fe_mul(t, inv_zz_zzz, r.zz);           // 1 / ZZZ
            fe_mul(y, r.y, t);                     // x, y: class F
        }
        g1_compress_point(o, x, y, r.inf);
        out[2 * i] = make_uint4(o[0], o[1], o[2], o[3]);
        out[2 * i + 1] = make_uint4(o[4], o[5], o[6], o[7]);
        return;
    }
    uint32_t o[16];
    if (r.inf) {
#pragma unroll
        for (int j = 0; j < 16; ++j) o[j] = 0;
    } else {
        Fq t, x, y;
        fe_mul(t, inv_zz_zzz, r.zzz);              // 1 / ZZ
        fe_mul(x, r.x, t);
        fe_mul(t, inv_zz_zzz, r.zz);               // 1 / ZZZ
        fe_mul(y, r.y, t);
        if (wire) {
            fe_norm(x); fe_norm(y);
            fe_to_wire(o, x);
            fe_to_wire(o + 8, y);
        } else {                                   // device affine format (curve.h): canonical residues of the internal form
            fe_canon(x); fe_canon(y);
            fe_pack(o, x);
            fe_pack(o + 8, y);
        }
    }
    out[4 * i] = make_uint4(o[0], o[1], o[2], o[3]);
    out[4 * i + 1] = make_uint4(o[4], o[5], o[6], o[7]);
    out[4 * i + 2] = make_uint4(o[8], o[9], o[10], o[11]);
    out[4 * i + 3] = make_uint4(o[12], o[13], o[14], o[15]);
}
// lane t converts the points i = t, t + T, t + 2T, ... (T = number of lanes) with ONE inversion (Montgomery's trick): prefix
// products of the denominators ZZ ZZZ go through `scratch` (9 limb planes, stride n).  per lane <= AFF_PER points.
constexpr uint32_t AFF_PER = 4;        // 16 while the lane's inversion was a 381-product chain; with division steps (fe_invert.h) shorter chains on more lanes win: 84 -> ~45 us at 1 024 points
template <bool BYTES = false>
__global__ void __launch_bounds__(256)
k_g1fft_to_affine(const int32_t* __restrict__ planes, uint32_t n, uint4* __restrict__ out, int wire, int32_t* __restrict__ scratch,
                  size_t planes_batch /* words between the plane sets of a batch (grid.y); its outputs and scratch rows are consecutive */) {
    planes += blockIdx.y * planes_batch;
    out += (size_t)blockIdx.y * (BYTES ? 2 : 4) * n;
    scratch += (size_t)blockIdx.y * NL * n;
    const uint32_t T = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    Fq run;
    fe_set_one(run);
    for (uint32_t i = t; i < n; i += T) {                 // forward: prefix products (identity points contribute 1)
        Xyzz v;
        xyzz_load(v, planes, n, i);
        Fq d;
        if (v.inf) fe_set_one(d); else fe_mul(d, v.zz, v.zzz);
#pragma unroll
        for (int j = 0; j < NL; ++j) scratch[(size_t)j * n + i] = run.l[j];
        fe_mul(run, run, d);
    }
    Fq rinv;
    fe_inverse_safegcd(rinv, run);                          // the ONE inversion behind every batched affine conversion: Bernstein-Yang division steps (fe_invert.h), ~20 us on a lone lane
    const uint32_t cnt = (n - 1 - t) / T + 1;
    for (uint32_t k = cnt; k-- > 0;) {                    // backward: inv_i = rinv * prefix_i; rinv *= d_i
        const uint32_t i = t + k * T;
        Xyzz v;
        xyzz_load(v, planes, n, i);
        Fq pre, d, iv;
#pragma unroll
        for (int j = 0; j < NL; ++j) pre.l[j] = scratch[(size_t)j * n + i];
        if (v.inf) fe_set_one(d); else fe_mul(d, v.zz, v.zzz);
        fe_mul(iv, rinv, pre);
        fe_mul(rinv, rinv, d);
        affine_emit<BYTES>(out, i, v, iv, wire != 0);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
struct ScalKey { int dev, log_n, scaled; bool operator<(const ScalKey& o) const { return dev != o.dev ? dev < o.dev : (log_n != o.log_n ? log_n < o.log_n : scaled < o.scaled); } };   // scaled: bit 0 = times 1/n, bits 1-2 = canon, bit 3 = forward (w^+e)
static std::map<ScalKey, uint4*> g_scal;
static std::mutex g_scal_mu;
// key_bits (g1fft_plan.h): G1SCAL_SCALED, canon in bits 1-2 (0 GLV halves, 1 canonical integers, 2 wire words), G1SCAL_FORWARD: the scalars of w^+e
// (the forward transform of g1_fft_planes) instead of w^-e; the kernel reads whichever table it is given
static int32_t get_scalars(kzg_ctx* ctx, int log_n, int key_bits, const uint4** out) {
    const bool scaled = (key_bits & G1SCAL_SCALED) != 0, forward = (key_bits & G1SCAL_FORWARD) != 0;
    const int canon = (key_bits >> 1) & 3;
    std::lock_guard<std::mutex> lk(g_scal_mu);
    ScalKey key{ctx->device, log_n, key_bits};
    auto it = g_scal.find(key);
    if (it != g_scal.end()) { *out = it->second; return KZG_OK; }
    NttTables tb{};
    if (log_n > 0) { int32_t rc = ntt_get_tables(ctx, log_n, !forward, &tb); if (rc != KZG_OK) return rc; }
    const size_t n = (size_t)1 << log_n;
    uint4* p = nullptr;
    KZG_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&p), n * 32));
    hipLaunchKernelGGL(k_g1fft_scalars, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, p, (uint32_t)n, log_n, tb, scaled ? 1 : 0, canon);
    KZG_HIP_TRY(ctx, hipGetLastError());
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    g_scal[key] = p;
    *out = p;
    return KZG_OK;
}

// width-3 NAF digit lists of the n scalars w^-e / n (scaled: the whole transform) or w^-e (a first stage), k_g1fft_naf2; cached per (device, log n, scaled)
struct Naf2Lists { uint16_t* list = nullptr; uint32_t* cnt = nullptr; };
static std::map<std::tuple<int, int, int>, Naf2Lists> g_naf2;
static int32_t get_naf2(kzg_ctx* ctx, int log_n, bool scaled, Naf2Lists* out) {
    const uint4* sc = nullptr;
    int32_t rc = get_scalars(ctx, log_n, G1SCAL_CANON | (scaled ? G1SCAL_SCALED : 0), &sc);            // canonical integers
    if (rc != KZG_OK) return rc;
    std::lock_guard<std::mutex> lk(g_scal_mu);
    auto key = std::make_tuple(ctx->device, log_n, scaled ? 1 : 0);
    auto it = g_naf2.find(key);
    if (it != g_naf2.end()) { *out = it->second; return KZG_OK; }
    const size_t n = (size_t)1 << log_n;
    Naf2Lists l;
    KZG_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&l.list), n * NAF2_MAX * 2));
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&l.cnt), n * 4);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_g1fft_naf2, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, sc, (uint32_t)n, l.list, l.cnt);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // shared by every context of the device: complete before it is published
    if (e != hipSuccess) { (void)hipFree(l.list); if (l.cnt) (void)hipFree(l.cnt); return set_error(ctx, e, "recoding the scalars of g1_ifft"); }
    g_naf2[key] = l;
    *out = l;
    return KZG_OK;
}

// XYZZ planes -> wire XYZZ words (32 u32 per point) for the host-side affine conversion of small transforms
__global__ void __launch_bounds__(256)
k_g1fft_planes_to_wire(const int32_t* __restrict__ planes, uint32_t n, uint32_t* __restrict__ out_wire) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Xyzz v;
    xyzz_load(v, planes, n, i);
    uint32_t w[32];
    xyzz_to_wire(w, v);
#pragma unroll
    for (int j = 0; j < 32; j += 4) *reinterpret_cast<uint4*>(out_wire + (size_t)i * 32 + j) = make_uint4(w[j], w[j + 1], w[j + 2], w[j + 3]);
}

// dst[i] = src[j], j = i or bit-reversed i, 36 limb planes each (src: element j of limb plane k at src[k * src_stride + j])
__global__ void __launch_bounds__(256)
k_g1fft_gather_planes(const int32_t* __restrict__ src, size_t src_stride, uint32_t n, int32_t* __restrict__ dst, int bitrev_log,
                      size_t src_batch, size_t dst_batch) {
    src += blockIdx.y * src_batch;
    dst += blockIdx.y * dst_batch;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = bitrev_log > 0 ? (__brev(i) >> (32 - bitrev_log)) : i;
#pragma unroll
    for (int k = 0; k < 4 * NL; ++k) dst[(size_t)k * n + i] = src[(size_t)k * src_stride + j];
}

// ---- a zero-padded input (g1_fft_planes_padded): only the first `nonzero` points of src exist, the identity stands after them ----------
// dst[i] = src[i] for i < nonzero, the identity (literal zeros) for nonzero <= i < n: the input copy of the direct stages
__global__ void __launch_bounds__(256)
k_g1fft_pad_planes(const int32_t* __restrict__ src, size_t src_stride, uint32_t nonzero, uint32_t n, int32_t* __restrict__ dst,
                   size_t src_batch, size_t dst_batch) {
    src += blockIdx.y * src_batch;
    dst += blockIdx.y * dst_batch;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int k = 0; k < 4 * NL; ++k) dst[(size_t)k * n + i] = i < nonzero ? src[(size_t)k * src_stride + i] : 0;
}

// The spread load: dst[i] = src[bitrev_{log_nonzero}(i >> log_r)], i < n = 2^(log_nonzero + log_r), one lane per output point.  In
// bit-reversed order the non-zero inputs of the radix-2 form stand on the multiples of r = 2^log_r, and the stages 1 .. log_r are
// butterflies (A, 0) -> (A, A): after them every run of r consecutive points holds one input, which is what this load writes.
__global__ void __launch_bounds__(256)
k_g1fft_spread_planes(const int32_t* __restrict__ src, size_t src_stride, uint32_t n, int log_nonzero, int log_r, int32_t* __restrict__ dst,
                      size_t src_batch, size_t dst_batch) {
    src += blockIdx.y * src_batch;
    dst += blockIdx.y * dst_batch;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t q = i >> log_r;                                 // < 2^log_nonzero
    const uint32_t j = log_nonzero > 0 ? (__brev(q) >> (32 - log_nonzero)) : 0;
#pragma unroll
    for (int k = 0; k < 4 * NL; ++k) dst[(size_t)k * n + i] = src[(size_t)k * src_stride + j];
}

// n XYZZ planes (stride n) -> n affine points (wire, or the device format of curve.h; identity = zeros), the batched conversion of
// g1_ifft_device; scratch: n x NL words.  Enqueued on st.
// batch plane sets planes_batch words apart (one per grid.y): point i of set b goes to d_out[b n + i], scratch: batch x n x NL words.
// compressed: the points leave as 32 gnark-compressed bytes each (point i of set b at d_out + 2 (b n + i)); `wire` is then unused.
int32_t g1fft_planes_to_affine(kzg_ctx* ctx, hipStream_t st, const int32_t* planes, size_t n, uint4* d_out, bool wire, int32_t* scratch, size_t batch, size_t planes_batch,
                               bool compressed) {
    const size_t lanes = std::max<size_t>(1, (n + AFF_PER - 1) / AFF_PER);
    const unsigned blocks = (unsigned)std::min<size_t>((lanes + 255) / 256, 4096);
    if (compressed) hipLaunchKernelGGL(k_g1fft_to_affine<true>, dim3(blocks, (unsigned)batch), dim3(256), 0, st, planes, (uint32_t)n, d_out, 0, scratch, planes_batch);
    else hipLaunchKernelGGL(k_g1fft_to_affine<false>, dim3(blocks, (unsigned)batch), dim3(256), 0, st, planes, (uint32_t)n, d_out, wire ? 1 : 0, scratch, planes_batch);
    KZG_HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

// ---- the driver: plan (g1fft_plan.h), fetch the tables the plan names, reserve from its sizes, walk its stages -----------------------------------
// what the stages of a plan read and write
struct G1fftOperands {
    const uint4* points = nullptr;                  // load: the SRS points
    const int32_t* in = nullptr;                    // gather, or the first direct stage of an unstrided transform: the caller's planes
    size_t in_stride = 0;
    int32_t* buf[2] = {nullptr, nullptr};           // the two plane sets
    int32_t* partial = nullptr;                     // partial sums (bits, first-tables, quad stages)
    const uint4* scal[G1SCAL_KEYS] = {};            // scalar tables by key
    uint32_t srs_n = 0;                             // SRS length: the stride of its tables
    const uint4* d_bits = nullptr;                  // bits stage: per-bit tables, their x3 / x5 / x7 tables, the digit lists
    const uint4* d_t3 = nullptr;
    uint32_t t3_points = 0;
    Naf2Lists nl;
    const uint4* tab = nullptr;                     // first-tables stage: the window tables
    uint32_t nonzero = 0;                           // pad / spread load: the points the input has
    int log_nonzero = 0;
    size_t in_batch = 0, buf_batch[2] = {0, 0};     // a batch (G1fftPlan::batch > 1): words between consecutive transforms' plane sets in `in` and in the two buffers
};

static int32_t g1fft_fetch_scalars(kzg_ctx* ctx, const G1fftPlan& p, G1fftOperands& io) {
    for (int i = 0; i < p.n_scal_keys; ++i) {
        int32_t rc = get_scalars(ctx, p.log_n, p.scal_keys[i], &io.scal[p.scal_keys[i]]);
        if (rc != KZG_OK) return rc;
    }
    return KZG_OK;
}

// every stage of the plan, enqueued on st
static int32_t g1fft_launch(kzg_ctx* ctx, hipStream_t st, const G1fftPlan& p, const G1fftOperands& io) {
    const uint32_t n = p.n;
    const int log_n = p.log_n;
    const dim3 block(256);
    for (int i = 0; i < p.n_stages; ++i) {
        const G1fftStage& s = p.stage[i];
        const dim3 grid((unsigned)s.grid, p.batch);                  // only the plane-to-plane kernels take a batch (the planner gives no other form one)
        const int32_t* src = s.src == G1BUF_INPUT ? io.in : io.buf[s.src];
        int32_t* dst = io.buf[s.dst];
        const size_t src_batch = s.src == G1BUF_INPUT ? io.in_batch : io.buf_batch[s.src], dst_batch = io.buf_batch[s.dst];
        const uint4* scal = s.scal >= 0 ? io.scal[s.scal] : nullptr;
        const int last = s.last ? 1 : 0;
        switch (s.kind) {
        case G1S_LOAD: case G1S_LOAD_BITREV:
            hipLaunchKernelGGL(k_g1fft_load, grid, block, 0, st, io.points, n, dst, s.kind == G1S_LOAD_BITREV ? log_n : 0);
            break;
        case G1S_GATHER: case G1S_GATHER_BITREV:
            hipLaunchKernelGGL(k_g1fft_gather_planes, grid, block, 0, st, io.in, io.in_stride, n, dst, s.kind == G1S_GATHER_BITREV ? log_n : 0, io.in_batch, dst_batch);
            break;
        case G1S_BITS:
            hipLaunchKernelGGL(k_g1fft_bits, grid, block, 0, st, io.d_bits, io.srs_n, io.d_t3, io.t3_points, n, log_n, s.K, io.nl.list, io.nl.cnt, s.Q, s.wpo, io.partial);
            break;
        case G1S_FIRST_TABLES:
            hipLaunchKernelGGL(k_g1fft_first_tables, grid, block, 0, st, io.tab, io.srs_n, p.tab_c, p.tab_W, n, log_n, s.K, scal, s.wpo, io.partial);
            break;
        case G1S_DIRECT:
            hipLaunchKernelGGL(k_g1fft_direct, grid, block, 0, st, src, dst, n, log_n, s.K, s.log_s, scal, last, src_batch, dst_batch);
            break;
        case G1S_DIRECT_PAIRS:
            hipLaunchKernelGGL(k_g1fft_direct_pairs, grid, block, 0, st, src, dst, n, log_n, s.K, s.log_s, scal, last, src_batch, dst_batch);
            break;
        case G1S_MUL_QUADS:
            hipLaunchKernelGGL(k_g1fft_mul_quads, grid, block, 0, st, src, io.partial, n, log_n, s.K, s.log_s, scal, last);
            break;
        case G1S_RADIX2:
            hipLaunchKernelGGL(k_g1fft_stage, grid, block, 0, st, dst, n, log_n, s.log_s, scal, last, dst_batch);
            break;
        case G1S_RADIX2_PAIRS:
            hipLaunchKernelGGL(k_g1fft_stage_pairs, grid, block, 0, st, dst, n, log_n, s.log_s, scal, last, dst_batch);
            break;
        case G1S_GATHER_PAD:
            hipLaunchKernelGGL(k_g1fft_pad_planes, grid, block, 0, st, io.in, io.in_stride, io.nonzero, n, dst, io.in_batch, dst_batch);
            break;
        case G1S_SPREAD_BITREV:
            hipLaunchKernelGGL(k_g1fft_spread_planes, grid, block, 0, st, io.in, io.in_stride, n, io.log_nonzero, s.log_s, dst, io.in_batch, dst_batch);
            break;
        case G1S_KINDS:
            break;
        }
        if (s.partials) hipLaunchKernelGGL(k_g1fft_sum_partials, dim3((unsigned)p.sum_grid), block, 0, st, io.partial, s.partials, n, dst);
    }
    KZG_HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

// The x3, x5, x7 tables of the first `pts` = min(SRS length, 2048) points, once per SRS (100 MB at 2 048 points), built and published under lazy_mu
static int32_t g1fft_t3_tables(kzg_ctx* ctx, const kzg_srs* srs, const uint4* d_bits, uint32_t pts, G1fftOperands& io) {
    std::unique_lock<std::mutex> lazy(srs->lazy_mu);
    if (!srs->d_t3) {
        hipStream_t st = ctx->stream;
        const uint32_t total = 3 * 255 * pts;
        KZG_HIP_TRY(ctx, ctx->poly[0].c.reserve((size_t)total * 36 * 4));
        KZG_HIP_TRY(ctx, ctx->poly[0].a.reserve((size_t)total * NL * 4));
        uint4* t3 = nullptr;
        KZG_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&t3), (size_t)total * 64));
        hipError_t e = hipMemsetAsync(t3, 0, (size_t)total * 64, st);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_g1fft_t3_planes, dim3((total + 255) / 256), dim3(256), 0, st, d_bits, (uint32_t)srs->n, pts, total, ctx->poly[0].c.as<int32_t>());
            const size_t lanes = (total + AFF_PER - 1) / AFF_PER;
            hipLaunchKernelGGL(k_g1fft_to_affine<false>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, ctx->poly[0].c.as<int32_t>(), total, t3, 0, ctx->poly[0].a.as<int32_t>(), (size_t)0);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { (void)hipFree(t3); return set_error(ctx, e, "building the x3 tables of g1_ifft"); }
        srs->d_t3 = t3;
        srs->t3_n = pts;
    }
    io.d_t3 = srs->d_t3;
    io.t3_points = srs->t3_n;
    return KZG_OK;
}

// The stages of the transform: *result_out = XYZZ planes (stride n) of the Lagrange basis of the first n SRS points, natural order
static int32_t g1_ifft_stages(kzg_ctx* ctx, const kzg_srs* srs, size_t n, const int32_t** result_out) {
    G1fftOperands io;
    io.d_bits = srs_bits(srs);
    G1fftSrsShape shape;
    shape.n = srs->n;
    shape.monomial = srs->lagrange_of == 0;
    shape.bit_tables = io.d_bits != nullptr;
    if (srs->d_small) { shape.small_c = srs->small_c; shape.small_W = srs->small_W; }
    shape.pre_c = srs->pre_c;
    shape.pre_W = srs->pre_W;
    const G1fftPlan p = g1fft_plan_ifft(n, shape);
    int32_t rc = g1fft_fetch_scalars(ctx, p, io);
    if (rc == KZG_OK && p.t3) rc = g1fft_t3_tables(ctx, srs, io.d_bits, p.t3_points, io);
    if (rc == KZG_OK && p.naf) rc = get_naf2(ctx, p.log_n, p.naf == 2, &io.nl);
    if (rc != KZG_OK) return rc;
    KZG_HIP_TRY(ctx, ctx->poly[0].a.reserve(p.bytes_a));
    KZG_HIP_TRY(ctx, ctx->poly[0].b.reserve(p.bytes_b));
    KZG_HIP_TRY(ctx, ctx->poly[0].c.reserve(p.bytes_c));
    io.points = srs->d_points;
    io.srs_n = (uint32_t)srs->n;
    io.tab = p.tab_small ? srs->d_small : srs->d_points;
    io.buf[0] = ctx->poly[0].b.as<int32_t>();
    io.buf[1] = io.buf[0] + n * 36;
    io.partial = ctx->poly[0].c.as<int32_t>();
    rc = g1fft_launch(ctx, ctx->stream, p, io);
    *result_out = io.buf[p.result];
    return rc;
}

// Lagrange basis of the first n SRS points -> d_out (n affine points: wire format, or the device format of curve.h)
int32_t g1_ifft_device(kzg_ctx* ctx, const kzg_srs* srs, size_t n, uint4* d_out, bool wire) {
    const int32_t* result = nullptr;
    int32_t rc = g1_ifft_stages(ctx, srs, n, &result);
    if (rc != KZG_OK) return rc;
    return g1fft_planes_to_affine(ctx, ctx->stream, result, n, d_out, wire, ctx->poly[0].a.as<int32_t>());
}

// ---- the generic transform (planes in, planes out): the FK20 multi-proofs of multiproof.hip --------------------------------------
// out = sum_j w^(+-ij) in[j] (times 1/n if scaled), natural order, n a power of two.  in: n points of XYZZ planes with stride in_stride
// (in_stride > n: a slice of a longer plane set, read in place by the radix-2 path's bit reversal, copied once for the direct stages);
// out, tmp: n points each, stride n, neither aliasing in.  The stage plan, the kernels and the scalar tables are g1_ifft's
// (g1fft_plan.h: the direct stages on lanes or pairs, radix-2 butterflies); forward transforms use the tables of w^+e.
// Enqueued on st; no synchronisation.
// A batch (b.batch > 1): that many transforms per launch, transform t reading in + t b.in_batch and leaving out + t b.out_batch (words;
// tmp likewise); the stage plan is chosen for the batch (g1fft_plan.h).
int32_t g1_fft_planes(kzg_ctx* ctx, hipStream_t st, const int32_t* in, size_t in_stride, size_t n, int32_t* out, int32_t* tmp, bool inverse, bool scaled, const G1fftBatch& b) {
    const G1fftPlan p = g1fft_plan_planes(n, inverse, scaled, in_stride != n, b.batch);
    G1fftOperands io;
    int32_t rc = g1fft_fetch_scalars(ctx, p, io);
    if (rc != KZG_OK) return rc;
    io.in = in;
    io.in_stride = in_stride;
    io.in_batch = b.in_batch;
    io.buf[p.result] = out;                                                  // the plan's ping-pong ends in out
    io.buf[1 - p.result] = tmp;
    io.buf_batch[p.result] = b.out_batch;
    io.buf_batch[1 - p.result] = b.tmp_batch;
    return g1fft_launch(ctx, st, p, io);
}

// The forward, unscaled transform of g1_fft_planes for an input whose points from `nonzero` on are the identity and are NOT read:
// in holds `nonzero` points (a power of two, <= n) with stride in_stride.  The plan is host_encode.h's: the direct stages behind a
// copy that pads, or the spread load and the radix-2 stages log2(n / nonzero) + 1 .. log2 n, on lanes or lane pairs as
// g1fft_choose_plan says for n.  The same group elements as g1_fft_planes on the padded input.  Enqueued on st.
int32_t g1_fft_planes_padded(kzg_ctx* ctx, hipStream_t st, const int32_t* in, size_t in_stride, size_t nonzero, size_t n, int32_t* out, int32_t* tmp, const G1fftBatch& b) {
    const G1fftPaddedPlan pp = g1fft_plan_planes_padded(n, nonzero, b.batch);
    const G1fftPlan& p = pp.plan;
    G1fftOperands io;
    int32_t rc = g1fft_fetch_scalars(ctx, p, io);
    if (rc != KZG_OK) return rc;
    io.in = in;
    io.in_stride = in_stride;
    io.nonzero = pp.nonzero;
    io.log_nonzero = pp.log_nonzero;
    io.in_batch = b.in_batch;
    io.buf[p.result] = out;
    io.buf[1 - p.result] = tmp;
    io.buf_batch[p.result] = b.out_batch;
    io.buf_batch[1 - p.result] = b.tmp_batch;
    return g1fft_launch(ctx, st, p, io);
}

// Up to this many points the one inversion of the affine conversion runs on the HOST (Montgomery's trick over the n points, ~20 us):
// on the device it is a 380-multiplication chain on lone lanes, 0.2 ms whatever n -- two thirds of a g1_ifft of 2..32 points.
constexpr size_t G1FFT_HOST_AFFINE_MAX = 256;

// the last context of device `dev` is gone: free the scalar tables and digit lists g1_ifft cached for it
void g1fft_release_device_caches(int dev) {
    std::lock_guard<std::mutex> lk(g_scal_mu);
    for (auto it = g_scal.begin(); it != g_scal.end();) {
        if (it->first.dev == dev) { (void)hipFree(it->second); it = g_scal.erase(it); } else ++it;
    }
    for (auto it = g_naf2.begin(); it != g_naf2.end();) {
        if (std::get<0>(it->first) == dev) { (void)hipFree(it->second.list); (void)hipFree(it->second.cnt); it = g_naf2.erase(it); } else ++it;
    }
}

int32_t g1_ifft_run(kzg_ctx* ctx, const kzg_srs* srs, size_t n, uint64_t* out_xy) {
    // (the transform as n batched MSMs of n pairs over the per-bit tables -- round 3's form at 512 points, 1.08 ms -- lost to the table first stage + one quad
    // stage, 0.68 ms, and was removed in round 6: docs/history, profiles/r03_g1ifft.txt)
    if (n <= G1FFT_HOST_AFFINE_MAX) {
        const int32_t* result = nullptr;
        int32_t rc = g1_ifft_stages(ctx, srs, n, &result);
        if (rc != KZG_OK) return rc;
        KZG_HIP_TRY(ctx, ctx->msm.bases_wire.reserve(n * 128));
        hipLaunchKernelGGL(k_g1fft_planes_to_wire, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, result, (uint32_t)n, ctx->msm.bases_wire.as<uint32_t>());
        KZG_HIP_TRY(ctx, hipGetLastError());
        static thread_local std::vector<kzg_host::Xyzz> host_pts;
        host_pts.resize(n);
        KZG_HIP_TRY(ctx, hipMemcpyAsync(host_pts.data(), ctx->msm.bases_wire.p, n * 128, hipMemcpyDeviceToHost, ctx->stream));
        KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        kzg_host::xyzz_batch_to_affine(host_pts.data(), n, out_xy);
        return KZG_OK;
    }
    KZG_HIP_TRY(ctx, ctx->msm.bases_wire.reserve(n * 64));
    int32_t rc = g1_ifft_device(ctx, srs, n, ctx->msm.bases_wire.as<uint4>(), true);
    if (rc != KZG_OK) return rc;
    KZG_HIP_TRY(ctx, hipMemcpyAsync(out_xy, ctx->msm.bases_wire.p, n * 64, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KZG_OK;
}

}  // namespace kzg

#if defined(KZG_DEVICE_BOUND_CHECK)   // the device bound-check variant only (field29.h, `make boundcheck`)
#include "field29.h"
KZG_BOUND_CHECK_EXPORTS(g1fft)
#endif
