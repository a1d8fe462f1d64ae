// poly.hip — the O(n) polynomial work of KZG::compute_proof_impl (prover/src/kzg.rs:128-178) on the GPU:
//   y   = p(z)                    barycentric, primitives/src/helpers.rs:475-535 (incl. the z-on-domain early return :497-504)
//   q_i = (f_i - y) / (w^i - z)   kzg.rs:151-174
//   q_m = sum_{i != m} (f_i - y) w^i / (z (z - w^i))   when z = w^m, kzg.rs:237-260
// then the quotient is committed as MSM(srs, IFFT(q)) (see kzg_commit_eval_form).
// The reference performs one field inversion per division (2n-3n serial inversions); here all denominators w^i - z
// share ONE inversion, done on the host: the domain is a group, so the product of the denominators over a coset
// {j + k n/m : k < m} is known in closed form,
//     prod_k (w^(j + k n/m) - z) = (-1)^(m+1) (W^j - z^m),   W = w^m  (the m-th roots of W^j are exactly those w^..),
// i.e. it is again a denominator of the SAME problem on the m-times smaller domain at the point z^m.  Montgomery's trick needs
// the inverse of each group's product: that is the smaller problem's answer.  The recursion ends at 1 / (1 - z^n), which the
// host computes while it enqueues (one 254-bit exponentiation, ~15 us); the device only multiplies: ~3 products per element
// and level.  (Round 1 / first half of round 2: one Fermat inversion per lane, 381 dependent multiplies = 213 us on the
// critical path of every proof, whatever n.)  Results are identical field elements.
// Also: helpers::calculate_roots_of_unity (helpers.rs:553-589) and helpers::to_fr_array as kernels.  (The batched evaluations of batch
// verification are vbeval.hip's.)
#include "poly_common.h"
#include "proof_plan.h"    // the proof driver's policy, the staging layout (ProofStaging, ProofScalars) and the chain's scalar table

#include <algorithm>
#include <cstring>

namespace kzg {

static_assert(PROOF_NL == NL && PROOF_THREADS == POLY_THREADS, "proof_plan.h sizes the workspaces for these kernels");

// ---- K0: the inverses 1 / (W^j - Z) on a small domain, one workgroup ----------------------------------------------
// out[j] = 1 / (w^(j e) - z^e), j < N = 2^log_ns <= 4096, e = n / N; zt[a] = z^(2^a) (wire), zt[log_n + 1] = 1 / (1 - z^n).
// Level by level from the single value 1 / (1 - z^n), size s -> 2 s, in place in LDS: lane t < s owns the pair {t, t + s} of the
// 2s-point domain, whose elements are +-W^t:  d0 = W^t - Z, d1 = -W^t - Z, d0 d1 = -(W^2t - Z^2), so with g = the value of the
// coarser level  1/d0 = -g d1,  1/d1 = -g d0: two independent multiplies per level and lane, log2 N levels.
// A zero denominator (z on the domain, the case of compute_proof_with_known_z_fr_index) gets the inverse 1, as the callers expect;
// the other denominators of its group are Z (rho - 1) for the roots of unity rho != 1 of the group, so their inverses are Z^-1 times
// constants: the host supplies z^-(2^a) and 1/(i-1), -1/2, 1/(-i-1) with the other scalars (zt[log_n+2 ..]).  The value such a lane
// read from the coarser level was never valid and is not used.
constexpr int POLY_SMALL_THREADS = 1024;
constexpr uint32_t POLY_SMALL_MAX_LOG = PROOF_SMALL_MAX_LOG;
constexpr uint32_t POLY_SMALL_MAX = 1u << POLY_SMALL_MAX_LOG;
__global__ void __launch_bounds__(POLY_SMALL_THREADS)
k_poly_inv_small(const uint4* __restrict__ zt, int log_n, int log_ns, NttTables tb, int32_t* __restrict__ out /* planes, stride 2^log_ns */) {
    extern __shared__ int32_t lds_inv[];                      // NL planes of 2^log_ns
    __shared__ int32_t zl[(POLY_SMALL_MAX_LOG + 1) * NL];     // canonical z^(2^log_e) of every level
    const uint32_t t0 = threadIdx.x, N = 1u << log_ns;
    if (t0 == 0) {
        Fr top;
        wire_load(top, zt, (size_t)ProofStaging::zt_top(log_n));
#pragma unroll
        for (int j = 0; j < NL; ++j) lds_inv[(size_t)j * N] = top.l[j];
    }
    if ((int)t0 < log_ns) {                                   // level log_s = t0 works on the 2^(t0+1)-point domain
        Fr z;
        wire_load(z, zt, (size_t)ProofStaging::zt_pow(log_n - (int)t0 - 1));
        fe_canon(z);
#pragma unroll
        for (int j = 0; j < NL; ++j) zl[t0 * NL + j] = z.l[j];
    }
    __syncthreads();
    for (int log_s = 0; log_s < log_ns; ++log_s) {
        const uint32_t s = 1u << log_s;
        const int log_e = log_n - log_s - 1;                   // the 2s-point domain: generator w^(2^log_e), point z^(2^log_e)
        // part A, independent of the coarser level: the two denominators of each of this thread's lanes (at most two lanes)
        Fr d0[2], d1[2];
        Fr z;
#pragma unroll
        for (int j = 0; j < NL; ++j) z.l[j] = zl[log_s * NL + j];
        auto part_a = [&](int q) {
            const uint32_t t = t0 + q * POLY_SMALL_THREADS;
            if (t >= s) return;
            Fr w;
            domain_elem(w, tb, t << log_e);
            fe_canon(w);
            fe_sub(d0[q], w, z);                               // W^t - Z
            fe_neg(d1[q], w);
            fe_norm(d1[q]);
            fe_canon(d1[q]);                                   // -W^t, canonical
            fe_sub(d1[q], d1[q], z);
        };
        part_a(0);
        part_a(1);
        // part B
        auto part_b = [&](int q) {
            const uint32_t t = t0 + q * POLY_SMALL_THREADS;
            if (t >= s) return;
            Fr g, i0, i1;
#pragma unroll
            for (int j = 0; j < NL; ++j) g.l[j] = -lds_inv[(size_t)j * N + t];
            fe_norm(g);
            const bool z0 = fe_is_literal_zero(d0[q]), z1 = fe_is_literal_zero(d1[q]);
            if (__builtin_expect(z0 || z1, 0)) {               // +-W^t = Z: the other denominator is -2 Z, its inverse (-1/2) Z^-1 from the host's table
                Fr zi, c2, other;
                wire_load(zi, zt, (size_t)ProofStaging::zt_inv_pow(log_n, log_e));
                wire_load(c2, zt, (size_t)ProofStaging::zt_const(log_n, 1));
                fe_mul(other, zi, c2);
                fe_set_one(i0); fe_set_one(i1);
                if (!z0) i0 = other;
                if (!z1) i1 = other;
            } else {
                fe_mul2(i0, g, d1[q], i1, g, d0[q]);
            }
#pragma unroll
            for (int j = 0; j < NL; ++j) { lds_inv[(size_t)j * N + t] = i0.l[j]; lds_inv[(size_t)j * N + t + s] = i1.l[j]; }
        };
        part_b(0);
        part_b(1);
        __syncthreads();
    }
    for (uint32_t i = t0; i < N; i += POLY_SMALL_THREADS)
#pragma unroll
        for (int j = 0; j < NL; ++j) out[(size_t)j * N + i] = lds_inv[(size_t)j * N + i];
}

// The four inverses of the coset {t + k T : k < 4} of the 4T-point domain (generator w^(2^log_e), point Z = z^(2^log_e), canonical):
// its elements are W^t times the fourth roots of unity 1, i, -1, -i (i = w^(n/4)), and d0 d1 d2 d3 = -(W^4t - Z^4), so with
// G = -next[t]:  1/d0 = G d1 (d2 d3),  1/d1 = G d0 (d2 d3),  1/d2 = G (d0 d1) d3,  1/d3 = G (d0 d1) d2.
// Returns the index k of a zero denominator (z on the domain; its inverse is set to 1), or 4.
__device__ __forceinline__ uint32_t inv4_group(Fr inv[4], const NttTables& tb, const uint4* __restrict__ zt, int log_n, int log_e, uint32_t t, const Fr& z,
                                               const int32_t* __restrict__ next, size_t next_stride) {
    Fr w0, w1, qi, d[4];
    domain_elem(w0, tb, t << log_e);
    domain_elem(qi, tb, 1u << (log_n - 2));                    // w^(n/4): the primitive fourth root
    fe_mul(w1, w0, qi);
    fe_canon(w0);
    fe_canon(w1);
    fe_sub(d[0], w0, z);
    fe_sub(d[1], w1, z);
    Fr n0, n1;
    fe_neg(n0, w0); fe_norm(n0); fe_canon(n0);
    fe_neg(n1, w1); fe_norm(n1); fe_canon(n1);
    fe_sub(d[2], n0, z);
    fe_sub(d[3], n1, z);
    uint32_t zero_k = 4;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) if (fe_is_literal_zero(d[k])) { zero_k = k; fe_set_one(d[k]); }
    if (__builtin_expect(zero_k != 4, 0)) {                    // d_k = Z (i^(k - k0) - 1): inverses = Z^-1 times the host's constants
        Fr zi;
        wire_load(zi, zt, (size_t)ProofStaging::zt_inv_pow(log_n, log_e));
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t r = (k - zero_k) & 3u;
            if (r == 0) { fe_set_one(inv[k]); continue; }
            Fr c;
            wire_load(c, zt, (size_t)(ProofStaging::zt_const(log_n, 0) + (r - 1)));
            fe_mul(inv[k], zi, c);
        }
        return zero_k;
    }
    Fr p01, p23, G;
    fe_mul2(p01, d[0], d[1], p23, d[2], d[3]);
    pl_load(G, next, next_stride, t);
    fe_neg(G, G);
    fe_norm(G);
    Fr a, b;
    fe_mul2(a, G, p23, b, G, p01);
    fe_mul2(inv[0], a, d[1], inv[1], a, d[0]);
    fe_mul2(inv[2], b, d[3], inv[3], b, d[2]);
    return zero_k;
}

// ---- K0b: one x4 level for domains too large for K0 --------------------------------------------------------------------
// out[j] = 1 / (w^(j e) - z^e), j < N = 2^log_nl, e = n / N, from next[t] = 1 / (w^(4 t e) - z^(4 e)), t < N / 4
__global__ void __launch_bounds__(POLY_THREADS)
k_poly_inv_level(const uint4* __restrict__ zt, int log_n, int log_nl, NttTables tb, const int32_t* __restrict__ next, int32_t* __restrict__ out) {
    const uint32_t N = 1u << log_nl, T = N >> 2, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const int log_e = log_n - log_nl;
    Fr z, inv[4];
    wire_load(z, zt, (size_t)ProofStaging::zt_pow(log_e));
    fe_canon(z);
    inv4_group(inv, tb, zt, log_n, log_e, t, z, next, T);
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) pl_store(out, N, t + k * T, inv[k]);
}

// y (reduced) into the proof's scalar image: the limbs for k_poly_quotient, the wire form for the read-back; one thread
__device__ __forceinline__ void proof_store_y(ProofScalars* __restrict__ ps, const Fr& y) {
#pragma unroll
    for (int j = 0; j < NL; ++j) ps->y[j] = y.l[j];
    fe_to_wire(ps->y_wire, y);
}
// 1/z = w^(n-m) for z = w^m
__device__ __forceinline__ void proof_z_inverse(Fr& zinv, const NttTables& tb, uint32_t n, uint32_t m) { domain_elem(zinv, tb, (n - m) & (n - 1)); }
// the on-domain element q_m = -(1/z) sum, sum = sum_{i != m} q_i w^i (kzg.rs:237-260); one thread
__device__ __forceinline__ void proof_store_q_m(uint4* __restrict__ q_out, uint32_t m, const Fr& sum, const Fr& zinv) {
    Fr q;
    fe_mul(q, sum, zinv);
    fe_neg(q, q);
    fe_norm(q);
    wire_store(q_out, m, q);
}
// y = (z^n - 1) / n * sum  for z off the domain (helpers.rs:529-532), into the proof's scalar image; one thread
__device__ __forceinline__ void poly_store_y_off_domain(const Fr& sum, int log_n, const uint4* __restrict__ z_wire, ProofScalars* __restrict__ ps) {
    Fr y, z, zn, one, ninv;
    wire_load(z, z_wire, 0);
    zn = z;
    for (int k = 0; k < log_n; ++k) fe_sqr(zn, zn);          // z^n, n = 2^log_n
    fe_set_one(one);
    fe_sub(zn, zn, one);                           // in (-3m, 2m)
#pragma unroll
    for (int j = 0; j < NL; ++j) ninv.l[j] = (int32_t)FrParams::NINV[log_n * NL + j];
    fe_mul(y, sum, zn);
    fe_mul(y, y, ninv);
#pragma unroll
    for (int j = 0; j < NL; ++j) ps->y[j] = y.l[j];          // as proof_store_y, written out: through the call k_poly_inverses came out with
    fe_to_wire(ps->y_wire, y);                               // other registers, and a proof of 1 024 evaluations measured outside the parent's spread
}

// ---- K1: the last level (inverses of all n denominators) + barycentric partial sums ---------------------------------------
// lane t owns elements i = k * T + t.  inv[i] = 1 / (w^i - z)  (1 for the on-domain index).
//   direct != 0: next[i] already is that inverse (n <= 4096: K0 produced all of them); any number of lanes
//   direct == 0: T = n / 4 lanes and next[t] = 1 / (w^(4 t) - z^4) (inv4_group)
__global__ void __launch_bounds__(POLY_THREADS)
k_poly_inverses(const uint4* __restrict__ evals, uint32_t n, int log_n, NttTables tb, const uint4* __restrict__ z_wire,
                const int32_t* __restrict__ next, int direct, int32_t* __restrict__ inv, int32_t* __restrict__ partial /* NL x gridDim */,
                ProofScalars* __restrict__ ps, int finish_y /* one workgroup, z off the domain: it also does what k_poly_finish_y would */) {
    __shared__ int32_t lds[NL * POLY_THREADS];
    const uint32_t T = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    Fr z;
    wire_load(z, z_wire, 0);
    fe_canon(z);
    Fr sum;
    fe_set_zero(sum);
    if (direct) {
        uint32_t cnt = 0;
        for (uint32_t i = t; i < n; i += T, ++cnt) {
            Fr w, wc, d, iv, f, term;
            domain_elem(w, tb, i);
            wc = w;
            fe_canon(wc);
            fe_sub(d, wc, z);
            if (fe_is_literal_zero(d)) ps->on_domain_index = i;
            pl_load(iv, next, n, i);
            if (next != inv) pl_store(inv, n, i, iv);
            wire_load(f, evals, i);
            fe_mul(term, f, w);
            fe_mul(term, term, iv);
            fe_sub(sum, sum, term);                   // barycentric term f_i w^i / (z - w^i) = -(f_i w^i inv_i)
            fe_norm(sum);                             // |sum| grows by 2m per term
            if ((cnt & 31u) == 31u) fe_reduce(sum);
        }
    } else if (t < (n >> 2)) {
        const uint32_t Tq = n >> 2;
        Fr iv[4], f[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) wire_load(f[k], evals, t + k * Tq);          // in flight during the inversion arithmetic
        const uint32_t zero_k = inv4_group(iv, tb, z_wire, log_n, 0, t, z, next, Tq);
        if (zero_k != 4) ps->on_domain_index = t + zero_k * Tq;
        Fr w0, w1, qi;
        domain_elem(w0, tb, t);
        domain_elem(qi, tb, 1u << (log_n - 2));
        fe_mul(w1, w0, qi);
        Fr fw[4];
        fe_mul2(fw[0], f[0], w0, fw[2], f[2], w0);                                     // w^(t + 2 Tq) = -w^t
        fe_mul2(fw[1], f[1], w1, fw[3], f[3], w1);
        Fr tm[4];
        fe_mul2(tm[0], fw[0], iv[0], tm[2], fw[2], iv[2]);
        fe_mul2(tm[1], fw[1], iv[1], tm[3], fw[3], iv[3]);
        // sum = -(tm0 + tm1) + (tm2 + tm3): elements 2 and 3 carry the factor -1 of their root
        fe_sub(sum, tm[2], tm[0]);
        fe_add(sum, sum, tm[3]);
        fe_sub(sum, sum, tm[1]);
        fe_norm(sum);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) pl_store(inv, n, t + k * Tq, iv[k]);
    }
    fe_reduce(sum);
    block_sum(sum, lds);
    if (threadIdx.x != 0) return;
    if (finish_y) poly_store_y_off_domain(sum, log_n, z_wire, ps);
    else pl_store(partial, gridDim.x, blockIdx.x, sum);
}

// ---- K2: y ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(POLY_THREADS)
k_poly_finish_y(const uint4* __restrict__ evals, uint32_t n, int log_n, const uint4* __restrict__ z_wire,
                const int32_t* __restrict__ partial, uint32_t n_partial, ProofScalars* __restrict__ ps) {
    __shared__ int32_t lds[NL * POLY_THREADS];
    Fr sum;
    sum_partials(sum, partial, n_partial, lds);
    if (threadIdx.x != 0) return;
    const uint32_t m = ps->on_domain_index;
    if (m == NO_INDEX) {
        poly_store_y_off_domain(sum, log_n, z_wire, ps);
        return;
    }
    Fr y;
    wire_load(y, evals, m);                       // helpers.rs:497-504
    proof_store_y(ps, y);
}

// ---- K3: quotient evaluations -----------------------------------------------------------------------------
__global__ void __launch_bounds__(POLY_THREADS)
k_poly_quotient(const uint4* __restrict__ evals, uint32_t n, NttTables tb, const int32_t* __restrict__ inv,
                const ProofScalars* __restrict__ ps, uint4* __restrict__ q_out, int32_t* __restrict__ partial) {
    __shared__ int32_t lds[NL * POLY_THREADS];
    const uint32_t T = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t m = ps->on_domain_index;
    Fr y;
#pragma unroll
    for (int j = 0; j < NL; ++j) y.l[j] = ps->y[j];
    Fr sum;
    fe_set_zero(sum);
    uint32_t cnt = 0;
    for (uint32_t i = t; i < n; i += T, ++cnt) {
        if (i == m) continue;
        Fr f, iv, q;
        wire_load(f, evals, i);
        pl_load(iv, inv, n, i);
        fe_sub(f, f, y);                          // (-3m, 3m)
        fe_mul(q, f, iv);
        wire_store(q_out, i, q);
        if (m != NO_INDEX) {                      // kzg.rs:237-260: accumulate q_i w^i
            Fr w, term;
            domain_elem(w, tb, i);
            fe_mul(term, q, w);
            fe_add(sum, sum, term);
            fe_norm(sum);
            if (cnt % 32 == 31) fe_reduce(sum);
        }
    }
    if (m == NO_INDEX) return;                    // uniform across the grid
    fe_reduce(sum);
    block_sum(sum, lds);
    if (threadIdx.x == 0) pl_store(partial, gridDim.x, blockIdx.x, sum);
}

// ---- K4: on-domain element q_m = -(1/z) sum_{i != m} q_i w^i, 1/z = w^(n-m) -------------------------------------
__global__ void __launch_bounds__(POLY_THREADS)
k_poly_quotient_on_domain(uint32_t n, NttTables tb, const int32_t* __restrict__ partial, uint32_t n_partial,
                          const ProofScalars* __restrict__ ps, uint4* __restrict__ q_out) {
    __shared__ int32_t lds[NL * POLY_THREADS];
    const uint32_t m = ps->on_domain_index;
    if (m == NO_INDEX) return;
    Fr sum;
    sum_partials(sum, partial, n_partial, lds);
    if (threadIdx.x != 0) return;
    Fr zinv;
    proof_z_inverse(zinv, tb, n, m);
    proof_store_q_m(q_out, m, sum, zinv);
}

// ---- K3' / K4': z = w^m with m known on the host (compute_proof_with_known_z_fr_index, kzg.rs:237-260), n <= POLY_SMALL_MAX ---------
// The denominators of an on-domain point are the SAME set for every m:  w^i - w^m = w^m (w^(i-m) - 1), so with the per-domain table
// t1[k] = 1 / (w^k - 1) (built once per domain size by the inversion chain above at z = 1) the inverse is w^(n-m) t1[(i - m) mod n]: no
// inversion chain, no barycentric sum (y = f_m, helpers.rs:497-504): three kernels (46 + 15 + 6 us for 2 048 evaluations) less per proof.
__global__ void __launch_bounds__(POLY_THREADS)
k_poly_quotient_table(const uint4* __restrict__ evals, uint32_t n, NttTables tb, const int32_t* __restrict__ t1, uint32_t m,
                      uint4* __restrict__ q_out, int32_t* __restrict__ partial, ProofScalars* __restrict__ ps /* one workgroup: it also finishes q_m and y */) {
    __shared__ int32_t lds[NL * POLY_THREADS];
    const uint32_t T = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    Fr y, zinv;
    wire_load(y, evals, m);
    fe_reduce(y);
    proof_z_inverse(zinv, tb, n, m);
    Fr sum;
    fe_set_zero(sum);
    uint32_t cnt = 0;
    for (uint32_t i = t; i < n; i += T, ++cnt) {
        if (i == m) continue;
        Fr f, iv, q, w, term;
        wire_load(f, evals, i);
        pl_load(iv, t1, n, (i - m) & (n - 1));
        fe_mul(iv, iv, zinv);                             // 1 / (w^i - w^m)
        fe_sub(f, f, y);                                  // (-3m, 3m)
        fe_mul(q, f, iv);
        wire_store(q_out, i, q);
        domain_elem(w, tb, i);
        fe_mul(term, q, w);
        fe_add(sum, sum, term);
        fe_norm(sum);
        if (cnt % 32 == 31) fe_reduce(sum);
    }
    fe_reduce(sum);
    block_sum(sum, lds);
    if (threadIdx.x != 0) return;
    if (gridDim.x > 1) { pl_store(partial, gridDim.x, blockIdx.x, sum); return; }
    proof_store_q_m(q_out, m, sum, zinv);                 // n <= 1 024: the only workgroup -- what k_poly_quotient_on_domain_known would do
    ps->on_domain_index = m;
    proof_store_y(ps, y);
}
// as K4, and y = f_m for the read-back
__global__ void __launch_bounds__(POLY_THREADS)
k_poly_quotient_on_domain_known(const uint4* __restrict__ evals, uint32_t n, NttTables tb, const int32_t* __restrict__ partial, uint32_t n_partial,
                                uint32_t m, ProofScalars* __restrict__ ps, uint4* __restrict__ q_out) {
    __shared__ int32_t lds[NL * POLY_THREADS];
    Fr sum;
    sum_partials(sum, partial, n_partial, lds);
    if (threadIdx.x != 0) return;
    Fr zinv, y;
    proof_z_inverse(zinv, tb, n, m);
    proof_store_q_m(q_out, m, sum, zinv);
    wire_load(y, evals, m);
    ps->on_domain_index = m;
    proof_store_y(ps, y);
}

// ---- blob bytes -> Fr (helpers::to_fr_array, primitives/src/helpers.rs:40-57) ---------------------------------------
// element i = the 32 big-endian bytes [32 i, 32 i + 32) (the last chunk right-padded with zeros) mod r, emitted in wire
// (Montgomery, radix 2^256) form; elements i >= n_elems (power-of-two padding of PolynomialEvalForm::new,
// polynomial.rs:49-51) are zero.  One multiply: x * (2^(256+261) mod r) * 2^-261 = x * 2^256 mod r, x < 2^256 < 5.3 r.
__global__ void __launch_bounds__(POLY_THREADS)
k_blob_to_fr(const uint8_t* __restrict__ bytes, size_t len, uint32_t n_elems, uint32_t n_padded, uint4* __restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_padded) return;
    uint32_t w32[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i < n_elems && (size_t)i * 32 + 32 <= len) {
        // a whole chunk (all but a ragged last one): two 16-byte loads and byte swaps instead of 32 single-byte loads -- 67 -> ~20 us at 2^20 elements
        // (the staging buffer comes from hipMalloc: 16-byte aligned)
        be_chunk_load(w32, bytes + (size_t)i * 32);
    } else if (i < n_elems) {
        const size_t base = (size_t)i * 32;
#pragma unroll
        for (int k = 0; k < 8; ++k) {              // word k (little-endian) = bytes 28-4k .. 31-4k of the big-endian chunk
            uint32_t w = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                size_t pos = base + (size_t)(28 - 4 * k + b);
                uint32_t byte = pos < len ? bytes[pos] : 0u;
                w = (w << 8) | byte;
            }
            w32[k] = w;
        }
    }
    Fr x, kk, r;
    fe_unpack(x, w32);
#pragma unroll
    for (int j = 0; j < NL; ++j) kk.l[j] = (int32_t)FrParams::K_RAW[j];       // 2^(256+261) mod r
    fe_mul(r, x, kk);                                                          // x * 2^256 mod r, in (-m, 2m)
    fe_canon(r);
    uint32_t o[8];
    fe_pack(o, r);
    out[2 * (size_t)i] = make_uint4(o[0], o[1], o[2], o[3]);
    out[2 * (size_t)i + 1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// ---- roots of unity -----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(POLY_THREADS)
k_poly_roots(uint4* __restrict__ out, uint32_t n, NttTables tb) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr w;
    domain_elem(w, tb, i);
    wire_store(out, i, w);
}

// ---- host -----------------------------------------------------------------------------------------------------
int32_t roots_run(kzg_ctx* ctx, uint64_t* out, size_t n) {
    int log_n = ilog2_ceil(n);
    NttTables tb;
    int32_t rc = ntt_get_tables(ctx, log_n, false, &tb);
    if (rc != KZG_OK) return rc;
    KZG_HIP_TRY(ctx, ctx->poly[0].a.reserve(n * 32));
    hipLaunchKernelGGL(k_poly_roots, dim3((unsigned)((n + POLY_THREADS - 1) / POLY_THREADS)), dim3(POLY_THREADS), 0, ctx->stream,
                       ctx->poly[0].a.as<uint4>(), (uint32_t)n, tb);
    KZG_HIP_TRY(ctx, hipGetLastError());
    KZG_HIP_TRY(ctx, hipMemcpyAsync(out, ctx->poly[0].a.p, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KZG_OK;
}

// bytes (host) -> n_padded wire elements (device).  Default buffers: ctx->poly[0].c (bytes), ctx->poly[0].a (elements), ctx->stream.
int32_t blob_to_fr_run(kzg_ctx* ctx, const uint8_t* bytes, size_t len, size_t n_padded, void** d_out,
                       hipStream_t st, DeviceBuffer* d_bytes, DeviceBuffer* d_elems) {
    if (!st) st = ctx->stream;
    if (!d_bytes) d_bytes = &ctx->poly[0].c;
    if (!d_elems) d_elems = &ctx->poly[0].a;
    const size_t n_elems = (len + 31) / 32;
    KZG_HIP_TRY(ctx, d_elems->reserve(n_padded * 32 + 32));
    KZG_HIP_TRY(ctx, d_bytes->reserve(len + 32));
    if (len) KZG_HIP_TRY(ctx, hipMemcpyAsync(d_bytes->p, bytes, len, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_blob_to_fr, dim3((unsigned)((n_padded + POLY_THREADS - 1) / POLY_THREADS)), dim3(POLY_THREADS), 0, st,
                       d_bytes->as<uint8_t>(), len, (uint32_t)n_elems, (uint32_t)n_padded, d_elems->as<uint4>());
    KZG_HIP_TRY(ctx, hipGetLastError());
    *d_out = d_elems->p;
    return KZG_OK;
}

// The known-index form's table 1 / (w^k - 1), k < n <= 4096, once per domain size: the inversion chain at z = 1
static int32_t proof_ondomain_table(kzg_ctx* ctx, int log_n, const NttTables& tb, hipStream_t st, const int32_t** out) {
    int32_t*& t1 = ctx->ondomain_inv[log_n];
    if (!t1) {
        const size_t n = (size_t)1 << log_n;
        uint64_t z1[ProofStaging::zt_count(PROOF_SMALL_MAX_LOG) * 4], one_w[4];
        const size_t z1_bytes = (size_t)ProofStaging::zt_count(log_n) * 32;
        bool on_domain;
        kzg_host::fr_one(one_w);
        proof_fill_scalars(one_w, log_n, z1, &on_domain);
        uint4* d_z1 = nullptr;
        KZG_HIP_TRY(ctx, hipMalloc(&d_z1, z1_bytes));
        hipError_t e1 = hipMalloc(&t1, (size_t)NL * n * 4);
        if (e1 == hipSuccess) e1 = hipMemcpy(d_z1, z1, z1_bytes, hipMemcpyHostToDevice);
        if (e1 == hipSuccess) {
            hipLaunchKernelGGL(k_poly_inv_small, dim3(1), dim3(POLY_SMALL_THREADS), (size_t)NL * n * 4, st, d_z1, log_n, log_n, tb, t1);
            e1 = hipGetLastError();
            if (e1 == hipSuccess) e1 = hipStreamSynchronize(st);
        }
        (void)hipFree(d_z1);
        if (e1 != hipSuccess) { if (t1) { (void)hipFree(t1); t1 = nullptr; } KZG_HIP_TRY(ctx, e1); }
    }
    *out = t1;
    return KZG_OK;
}

// What the steps of a plan work on
struct ProofOperands {
    const uint64_t* evals;        // host evaluations, or nullptr
    const uint4* d_a;             // the n evaluations on the device: set.a or the caller's buffer
    const int32_t* table;         // PROOF_FORM_TABLE: 1 / (w^k - 1)
    uint32_t m_known;             // ... and the index of z
    NttWorkspace* nttws;
};
// Walks the plan's steps: each kernel's launch, each copy and the join of the two streams are written here once
static int32_t proof_launch(kzg_ctx* ctx, PolySet& set, hipStream_t st, const ProofPlan& plan, const NttTables& tb, const ProofOperands& op) {
    const size_t n = (size_t)1 << plan.log_n;
    const int log_n = plan.log_n;
    const uint32_t blocks = plan.blocks;
    uint8_t* small = set.small.as<uint8_t>();
    uint8_t* pin = static_cast<uint8_t*>(set.pinned);
    ProofScalars* ps = reinterpret_cast<ProofScalars*>(small + ProofStaging::IMAGE);
    const uint4* d_zt = reinterpret_cast<const uint4*>(small + ProofStaging::ZT);      // its first element is z itself
    int32_t* partial = reinterpret_cast<int32_t*>(small + ProofStaging::PARTIALS);
    int32_t* d_inv = set.b.as<int32_t>();
    int32_t* d_lvl = d_inv + n * NL;
    uint4* d_q = set.c.as<uint4>();
    auto lvl = [&](size_t off) { return off == PROOF_OUT_INV ? d_inv : d_lvl + off; };
    hipStream_t sc = st;                                     // the chain's stream
    if (plan.aux) {
        int32_t rca = ctx_aux_stream(ctx, st, &sc);
        if (rca != KZG_OK) return rca;
    }
    ProofScalars* ps_out = nullptr;                          // the table form's kernels write the read-back slot themselves
    if (plan.form == PROOF_FORM_TABLE) {
        void* ps_host_dev = nullptr;
        KZG_HIP_TRY(ctx, hipHostGetDevicePointer(&ps_host_dev, pin + ProofStaging::Y_READBACK, 0));
        ps_out = static_cast<ProofScalars*>(ps_host_dev);
    }
    bool unchecked = false;                                  // a kernel was launched since the last hipGetLastError
    for (int i = 0; i < plan.n_steps; ++i) {
        const ProofStep& s = plan.step[i];
        if (unchecked && proof_step_collects_errors(s.kind)) {
            KZG_HIP_TRY(ctx, hipGetLastError());
            unchecked = false;
        }
        unchecked |= s.kind >= PS_FIRST_KERNEL;
        switch (s.kind) {
        case PS_UPLOAD_SCALARS:   // one upload for the scalar image and the chain's scalars right behind it
            KZG_HIP_TRY(ctx, hipMemcpyAsync(small, pin, ProofStaging::upload_bytes(log_n), hipMemcpyHostToDevice, sc));
            break;
        case PS_UPLOAD_EVALS:
            KZG_HIP_TRY(ctx, hipMemcpyAsync(set.a.p, op.evals, n * 32, hipMemcpyHostToDevice, st));
            break;
        case PS_INV_SMALL:
            hipLaunchKernelGGL(k_poly_inv_small, dim3(1), dim3(POLY_SMALL_THREADS), plan.small_lds, sc, d_zt, log_n, plan.small_log_ns, tb, lvl(plan.small_out));
            break;
        case PS_INV_LEVEL: {
            const ProofLevel& l = plan.level[s.level];
            const uint32_t T = 1u << (l.log_l - 2);
            hipLaunchKernelGGL(k_poly_inv_level, dim3((T + POLY_THREADS - 1) / POLY_THREADS), dim3(POLY_THREADS), 0, sc, d_zt, log_n, l.log_l, tb,
                               (const int32_t*)lvl(s.level + 1 < plan.n_levels ? plan.level[s.level + 1].off : plan.small_out), lvl(l.off));
            break;
        }
        case PS_RECORD_CHAIN:
            if (!set.ev_chain) KZG_HIP_TRY(ctx, hipEventCreateWithFlags(&set.ev_chain, hipEventDisableTiming));
            KZG_HIP_TRY(ctx, hipEventRecord(set.ev_chain, sc));
            break;
        case PS_JOIN_CHAIN:
            KZG_HIP_TRY(ctx, hipStreamWaitEvent(st, set.ev_chain, 0));
            break;
        case PS_INVERSES:
            hipLaunchKernelGGL(k_poly_inverses, dim3(blocks), dim3(POLY_THREADS), 0, st, op.d_a, (uint32_t)n, log_n, tb, d_zt,
                               (const int32_t*)lvl(plan.next_off), plan.direct, d_inv, partial, ps, (int)plan.fused_y);
            break;
        case PS_FINISH_Y:
            hipLaunchKernelGGL(k_poly_finish_y, dim3(1), dim3(POLY_THREADS), 0, st, op.d_a, (uint32_t)n, log_n, d_zt, partial, blocks, ps);
            break;
        case PS_READ_Y:
            KZG_HIP_TRY(ctx, hipMemcpyAsync(pin + ProofStaging::Y_READBACK, ps, sizeof(ProofScalars), hipMemcpyDeviceToHost, st));
            break;
        case PS_QUOTIENT:
            hipLaunchKernelGGL(k_poly_quotient, dim3(blocks), dim3(POLY_THREADS), 0, st, op.d_a, (uint32_t)n, tb, d_inv, ps, d_q, partial);
            break;
        case PS_QUOTIENT_ON_DOMAIN:
            hipLaunchKernelGGL(k_poly_quotient_on_domain, dim3(1), dim3(POLY_THREADS), 0, st, (uint32_t)n, tb, partial, blocks, ps, d_q);
            break;
        case PS_QUOTIENT_TABLE:
            hipLaunchKernelGGL(k_poly_quotient_table, dim3(blocks), dim3(POLY_THREADS), 0, st, op.d_a, (uint32_t)n, tb, op.table, op.m_known, d_q, partial, ps_out);
            break;
        case PS_QUOTIENT_KNOWN:
            hipLaunchKernelGGL(k_poly_quotient_on_domain_known, dim3(1), dim3(POLY_THREADS), 0, st, op.d_a, (uint32_t)n, tb, partial, blocks, op.m_known, ps_out, d_q);
            break;
        case PS_INTT:
            return ntt_run(ctx, set.c.p, n, true, st, op.nttws);
        }
    }
    if (unchecked) KZG_HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

// Enqueue the O(n) part of a proof on `st` with the buffers of `ps_set`, without waiting: upload, denominators + batch
// inversion, y, quotient (+ on-domain entry), IFFT of the quotient.  y is left in the read-back slot of ps_set.pinned (ProofStaging::Y_READBACK,
// valid once the stream has been synchronised); the quotient's coefficients are left in ps_set.c.
// skip_intt: the caller commits the quotient's EVALUATIONS over a Lagrange basis (prover/src/kzg.rs:96-100 applied to the quotient, exactly
// what the reference's compute_proof_impl does: kzg.rs:176-177), so they stay in set.c as they are.
// d_resident: the n evaluations (wire) already on the device in a buffer of the caller's (the jobs of blobstream.hip); read in place
// evals == nullptr without d_resident: set.a already holds the n evaluations (blob proofs)
// The driver: the chain's scalars (they say where z lies), plan (proof_plan.h), tables, the reserves from the plan, staging, the known-index
// table, the plan's steps.
static int32_t proof_enqueue(kzg_ctx* ctx, PolySet& set, hipStream_t st, NttWorkspace* nttws, const uint64_t* evals, size_t n,
                             const uint64_t z[4], bool want_proof, bool skip_intt = false, const uint4* d_resident = nullptr) {
    RoctxRange range(want_proof ? "kzg:proof:inverses + y + quotient + intt" : "kzg:evaluate:inverses + y");
    const int log_n = ilog2_ceil(n);
    uint64_t zt[ProofStaging::zt_count(PROOF_MAX_LOG) * 4];
    bool z_on_domain = false;
    proof_fill_scalars(z, log_n, zt, &z_on_domain);
    ProofOperands op{};
    op.evals = d_resident ? nullptr : evals;
    op.nttws = nttws;
    op.m_known = NO_INDEX;
    const bool index_known = proof_table_eligible(log_n, want_proof, z_on_domain) && kzg_host::fr_domain_index(z, log_n, &op.m_known);
    const ProofPlan plan = proof_plan(log_n, want_proof, skip_intt, z_on_domain, index_known,
                                      d_resident ? PROOF_EVALS_RESIDENT : evals ? PROOF_EVALS_HOST : PROOF_EVALS_IN_SET);
    NttTables tb;
    int32_t rc = ntt_get_tables(ctx, log_n, false, &tb);
    if (rc != KZG_OK) return rc;
    if (plan.intt && n > 1) { NttTables tbi; rc = ntt_get_tables(ctx, log_n, true, &tbi); if (rc != KZG_OK) return rc; }
    if (plan.bytes_a) KZG_HIP_TRY(ctx, set.a.reserve(plan.bytes_a));
    KZG_HIP_TRY(ctx, set.b.reserve(plan.bytes_b));
    KZG_HIP_TRY(ctx, set.c.reserve(plan.bytes_c));
    KZG_HIP_TRY(ctx, set.small.reserve(plan.bytes_small));
    if (!set.pinned) KZG_HIP_TRY(ctx, hipHostMalloc(&set.pinned, ProofStaging::PINNED_BYTES, hipHostMallocDefault));
    op.d_a = d_resident ? d_resident : set.a.as<uint4>();
    // the staging image: the initial ProofScalars, zero fill, the chain's scalars
    uint8_t* pin = static_cast<uint8_t*>(set.pinned);
    memset(pin + ProofStaging::IMAGE, 0, ProofStaging::IMAGE_BYTES);
    reinterpret_cast<ProofScalars*>(pin + ProofStaging::IMAGE)->on_domain_index = NO_INDEX;
    memcpy(pin + ProofStaging::ZT, zt, (size_t)ProofStaging::zt_count(log_n) * 32);
    if (!ctx->poly_lds_attr_set) {
        KZG_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_poly_inv_small), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(NL * POLY_SMALL_MAX * 4)));
        ctx->poly_lds_attr_set = true;
    }
    if (plan.form == PROOF_FORM_TABLE) {
        rc = proof_ondomain_table(ctx, log_n, tb, st, &op.table);
        if (rc != KZG_OK) return rc;
    }
    return proof_launch(ctx, set, st, plan, tb, op);
}
// The cached Lagrange basis of exactly n points, if the SRS carries one (without one: the IFFT + monomial-basis form)
static const kzg_srs* proof_lagrange_basis(const kzg_srs* srs, size_t n) {
    if (n < 2 || srs->lagrange_of != 0) return nullptr;
    return srs_cached_lagrange(srs, n);
}
static void proof_read_y(const PolySet& set, uint64_t* out_y) {
    const ProofScalars* host = reinterpret_cast<const ProofScalars*>(static_cast<const uint8_t*>(set.pinned) + ProofStaging::Y_READBACK);
    memcpy(out_y, host->y_wire, 32);
}

int32_t proof_run(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* evals, size_t n, const uint64_t z[4],
                  uint64_t out_xy[8], uint8_t* out_inf, uint64_t* out_y, bool want_proof, size_t coeff_lo, uint64_t* out_xyzz) {
    if (ctx->slot_pending[0]) {
        ctx->last_error = "a kzg_*_begin on slot 0 is still in flight: call its end first";
        return KZG_ERR_INVALID_ARG;
    }
    PolySet& set = ctx->poly[0];
    hipStream_t st = ctx->stream;
    // a Lagrange basis of n points cached with the SRS (kzg_srs_cache_lagrange): the quotient is committed in evaluation form, no IFFT
    const kzg_srs* lag = (want_proof && srs && coeff_lo == 0) ? proof_lagrange_basis(srs, n) : nullptr;
    int32_t rc = proof_enqueue(ctx, set, st, &ctx->ntt, evals, n, z, want_proof, lag != nullptr);
    if (rc != KZG_OK) { (void)hipStreamSynchronize(st); return rc; }
    if (lag) {
        rc = msm_run(ctx, srs_bases(lag, 0, n, ctx->msm_c_override == 0), set.c.p, n, out_xy, out_inf, out_xyzz);
    } else if (want_proof && coeff_lo < n) {
        // the whole SRS commits the whole quotient; a shard holding powers [coeff_lo, coeff_lo + srs->n) commits its slice of it
        const size_t len = std::min(srs->n, n - coeff_lo);
        rc = msm_run(ctx, srs_bases(srs, 0, len, ctx->msm_c_override == 0), set.c.as<uint4>() + 2 * coeff_lo, len, out_xy, out_inf, out_xyzz);
    } else {
        // nothing to commit: an evaluation only, or a shard past the quotient's end (its share is the identity)
        KZG_HIP_TRY(ctx, hipStreamSynchronize(st));
        if (want_proof) {
            if (out_xyzz) memset(out_xyzz, 0, 128);
            if (out_xy) { memset(out_xy, 0, 64); if (out_inf) *out_inf = 1; }
        }
    }
    if (rc == KZG_OK && out_y) proof_read_y(set, out_y);      // the stream is synchronised: by msm_run, or just above
    return rc;
}

// asynchronous form: everything on the slot's stream; proof_end collects the point and y
int32_t proof_begin(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* evals, size_t n, const uint64_t z[4], int slot, const void* d_resident) {
    if (slot < 0 || slot >= KZG_NUM_SLOTS || ctx->slot_pending[slot]) return KZG_ERR_INVALID_ARG;
    hipStream_t st = nullptr;
    int32_t rc = msm_slot_stream(ctx, slot, &st);
    if (rc != KZG_OK) return rc;
    PolySet& set = ctx->poly[slot];
    const kzg_srs* lag = proof_lagrange_basis(srs, n);
    rc = proof_enqueue(ctx, set, st, &ctx->slot_ntt(slot), evals, n, z, true, lag != nullptr, static_cast<const uint4*>(d_resident));
    if (rc != KZG_OK) { (void)hipStreamSynchronize(st); return rc; }
    return msm_begin(ctx, slot, srs_bases(lag ? lag : srs, 0, n, ctx->msm_c_override == 0), set.c.p, n);
}
int32_t proof_end(kzg_ctx* ctx, int slot, uint64_t out_xy[8], uint8_t* out_inf, uint64_t* out_y) {
    int32_t rc = msm_end(ctx, slot, out_xy, out_inf, nullptr);
    if (rc == KZG_OK && out_y) proof_read_y(ctx->poly[slot], out_y);
    return rc;
}

}  // namespace kzg

#if defined(KZG_DEVICE_BOUND_CHECK)   // the device bound-check variant only (field29.h, `make boundcheck`)
#include "field29.h"
KZG_BOUND_CHECK_EXPORTS(poly)
#endif
