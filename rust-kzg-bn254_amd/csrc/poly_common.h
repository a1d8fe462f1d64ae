// poly_common.h -- helpers shared by the polynomial kernels (poly.hip: whole-domain proofs; vbeval.hip: the batched evaluations of batch
// verification; recover.hip) and the evaluation-slice kernels of the Lagrange-sharded proofs (lagrange.hip): limb-plane loads / stores, domain
// elements from the two-level twiddle tables, wire <-> internal conversion, the big-endian chunk load, the workgroup sum and the sum of
// per-workgroup partials, Montgomery's trick across a workgroup, and host-side Fr arithmetic on wire words for the handful of
// scalars a proof needs on the host.
#pragma once
#include "engine.h"
#include "field29.h"
#include "host_fr.h"

#include <cstring>

namespace kzg {

constexpr int POLY_THREADS = 256;
constexpr uint32_t NO_INDEX = 0xFFFFFFFFu;

__device__ __forceinline__ void pl_load(Fr& v, const int32_t* __restrict__ planes, size_t stride, size_t i) {
#pragma unroll
    for (int j = 0; j < NL; ++j) v.l[j] = planes[(size_t)j * stride + i];
}
__device__ __forceinline__ void pl_store(int32_t* __restrict__ planes, size_t stride, size_t i, const Fr& v) {
#pragma unroll
    for (int j = 0; j < NL; ++j) planes[(size_t)j * stride + i] = v.l[j];
}
__device__ __forceinline__ void domain_elem(Fr& w, const NttTables& tb, uint32_t E) {   // w^E, result in (-m, 2m)
    pl_load(w, tb.lo, tb.lo_len, E & (tb.lo_len - 1));
    uint32_t eh = E >> tb.lo_bits;
    if (eh != 0) {
        Fr h;
        pl_load(h, tb.hi, tb.hi_len, eh);
        fe_mul(w, w, h);
    }
}
__device__ __forceinline__ void wire_load(Fr& v, const uint4* __restrict__ src, size_t i) {   // wire -> internal, (-m, 2m)
    uint4 a = src[2 * i], b = src[2 * i + 1];
    uint32_t w32[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    fe_from_wire(v, w32);
}
__device__ __forceinline__ void wire_store(uint4* __restrict__ dst, size_t i, const Fr& v) {  // internal (|v| < 169 m) -> wire
    uint32_t w32[8];
    fe_to_wire(w32, v);
    dst[2 * i] = make_uint4(w32[0], w32[1], w32[2], w32[3]);
    dst[2 * i + 1] = make_uint4(w32[4], w32[5], w32[6], w32[7]);
}
// block-wide sum of one Fr per thread (values in (-m, 2m)); result (reduced) valid in thread 0
__device__ __forceinline__ void block_sum(Fr& v, int32_t* lds /* NL * POLY_THREADS */) {
    const int t = threadIdx.x;
    int level = 0;
    for (int d = POLY_THREADS / 2; d >= 1; d >>= 1, ++level) {
#pragma unroll
        for (int j = 0; j < NL; ++j) lds[j * POLY_THREADS + t] = v.l[j];
        __syncthreads();
        if (t < d) {
            Fr u;
#pragma unroll
            for (int j = 0; j < NL; ++j) u.l[j] = lds[j * POLY_THREADS + t + d];
            fe_add(v, v, u);
            fe_norm(v);
            if (level == 3) fe_reduce(v);        // 16 terms so far: |v| < 32 m -> back to (-m, 2m)
        }
        __syncthreads();
    }
    if (t == 0) fe_reduce(v);
}
// sum of n_partial per-workgroup partials (limb planes, stride n_partial, values in (-m, 2m)) by ONE workgroup; result (reduced) valid in thread 0
__device__ __forceinline__ void sum_partials(Fr& sum, const int32_t* partial, uint32_t n_partial, int32_t* lds /* NL * POLY_THREADS */) {
    fe_set_zero(sum);
    for (uint32_t i = threadIdx.x; i < n_partial; i += POLY_THREADS) {
        Fr v;
        pl_load(v, partial, n_partial, i);
        fe_add(sum, sum, v);
        fe_norm(sum);
        if ((i / POLY_THREADS) % 32 == 31) fe_reduce(sum);
    }
    fe_reduce(sum);
    block_sum(sum, lds);
}
// the 32 big-endian bytes at p (16-byte aligned) as eight little-endian words: two 16-byte loads and byte swaps
__device__ __forceinline__ void be_chunk_load(uint32_t w32[8], const uint8_t* __restrict__ p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 hi = q[0], lo = q[1];              // bytes 0..15 (most significant), 16..31
    w32[7] = __builtin_bswap32(hi.x); w32[6] = __builtin_bswap32(hi.y); w32[5] = __builtin_bswap32(hi.z); w32[4] = __builtin_bswap32(hi.w);
    w32[3] = __builtin_bswap32(lo.x); w32[2] = __builtin_bswap32(lo.y); w32[1] = __builtin_bswap32(lo.z); w32[0] = __builtin_bswap32(lo.w);
}
// Montgomery's trick across a workgroup: lane t < Lf (a power of two) has stored its value at leaf Lf + t of `tree` (NL planes of 2 Lf
// nodes, heap order: root 1) and finds its inverse there on return.  Called by every lane of the workgroup.  root_inverse(ri, r) gives
// the inverse ri of the root product r on lane 0: the one inversion of the workgroup.  None of the values may be zero.
template <typename RootInverse>
__device__ __forceinline__ void lds_tree_invert(int32_t* tree, uint32_t Lf, uint32_t t, RootInverse root_inverse) {
    const uint32_t S = 2 * Lf;
    __syncthreads();
    for (uint32_t s = Lf >> 1; s >= 1; s >>= 1) {            // up-sweep: node = product of its two children
        if (t < s) {
            const uint32_t node = s + t;
            Fr a, c, r;
#pragma unroll
            for (int j = 0; j < NL; ++j) { a.l[j] = tree[j * S + 2 * node]; c.l[j] = tree[j * S + 2 * node + 1]; }
            fe_mul(r, a, c);
#pragma unroll
            for (int j = 0; j < NL; ++j) tree[j * S + node] = r.l[j];
        }
        __syncthreads();
    }
    if (t == 0) {
        Fr root, ri;
#pragma unroll
        for (int j = 0; j < NL; ++j) root.l[j] = tree[j * S + 1];
        root_inverse(ri, root);
#pragma unroll
        for (int j = 0; j < NL; ++j) tree[j * S + 1] = ri.l[j];
    }
    __syncthreads();
    for (uint32_t s = 1; s < Lf; s <<= 1) {                  // down-sweep: inverse of a child = inverse of the node x its sibling
        if (t < s) {
            const uint32_t node = s + t;
            Fr g, a, c, ia, ic;
#pragma unroll
            for (int j = 0; j < NL; ++j) { g.l[j] = tree[j * S + node]; a.l[j] = tree[j * S + 2 * node]; c.l[j] = tree[j * S + 2 * node + 1]; }
            fe_mul2(ia, g, c, ic, g, a);
#pragma unroll
            for (int j = 0; j < NL; ++j) { tree[j * S + 2 * node] = ia.l[j]; tree[j * S + 2 * node + 1] = ic.l[j]; }
        }
        __syncthreads();
    }
}

}  // namespace kzg
