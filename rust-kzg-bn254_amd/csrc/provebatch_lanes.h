// provebatch_lanes.h -- the lane code of the batched prover (provebatch.hip k_pb_prep / k_pb_prove): what ONE lane of a blob's workgroup does
// between two barriers, as plain functions of the lane index t and of the workgroup's shared planes.  The kernels call them with
// __syncthreads() in between; tests/hostcheck/provebatchcheck.cpp compiles the same functions with g++ -DKZG_BOUND_CHECK and runs a
// workgroup lane by lane (a barrier is the end of a loop over t).  Nothing here names a HIP type besides the 16-byte loads and stores of the
// device pass.
//
// One workgroup per polynomial of n = 2^log_n <= 2^PB_MAX_LOG evaluations f_j (wire form, row b of a rows x n array) and one point z:
//   y   = f(z)                                   (helpers.rs:485-532)
//   q_j = (f_j - y) / (w^j - z) = (y - f_j) / d_j, d_j = z - w^j         (kzg.rs:151-174)
// Lane t < Lf = min(n, PB_THREADS) owns the M = n / Lf in {1, 2, 4, 8} indices j = t + k Lf, as vbeval.hip's lanes do: the product of
// its denominators is a leaf of a product tree in shared memory, the root's inverse comes from k_pb_prep (the ONE inversion of the blob),
// the walk down leaves every lane the inverse of its product and Montgomery's trick inside the lane gives the M inverses.  They stay in
// REGISTERS (lane.d[k] is overwritten by 1 / d_k) across the block sum that gives y, with the M evaluations beside them, so the
// quotient row costs one subtraction, one product and one store per element after y is known.
//
// z on the domain, z = w^m (kzg.rs:237-260, helpers.rs:497-504): the lane that finds d_j = 0 puts 1 in its place and publishes m = j.  The
// root is then prod_{j != m} (w^m - w^j) = n w^(-m) = n / z (the derivative of X^n - 1 at w^m), whose inverse z / n k_pb_prep forms with one
// product and NO inversion; y = f_m; q_j as above for j != m; q_m = -(1/z) sum_{j != m} q_j w^j with 1/z = w^(n-m): one more block sum.
#pragma once
#include "field29.h"
#include "fe_invert.h"

namespace kzg {

constexpr int PB_THREADS = 512;          // lanes of the largest class's workgroup: 8 waves, two per SIMD (a class of n < 512 runs max(n, 64) lanes)
constexpr int PB_MAX_LOG = 12;           // n <= 8 PB_THREADS
constexpr uint32_t PB_NO_INDEX = 0xFFFFFFFFu;

// what k_pb_prep leaves for a blob's workgroup: z canonical (internal form), z^n - 1 in (-m, 2m), the inverse of the tree's root
struct PbPrep { int32_t z[NL]; int32_t znm1[NL]; int32_t tinv[NL]; uint32_t on_domain; };
// the words a workgroup shares besides the planes: y (internal form, (-m, 2m)) and the on-domain index
struct PbShared { int32_t y[NL]; uint32_t m; };

KZG_HD void pb_pl_load(Fr& v, const int32_t* planes, size_t stride, size_t i) {
#pragma unroll
    for (int j = 0; j < NL; ++j) v.l[j] = planes[(size_t)j * stride + i];
}
KZG_HD void pb_pl_store(int32_t* planes, size_t stride, size_t i, const Fr& v) {
#pragma unroll
    for (int j = 0; j < NL; ++j) planes[(size_t)j * stride + i] = v.l[j];
}
// w^E from two-level twiddle tables (TB: lo, lo_len, lo_bits, hi, hi_len as NttTables has them), result in (-m, 2m)
template <class TB>
KZG_HD void pb_domain_elem(Fr& w, const TB& tb, uint32_t E) {
    pb_pl_load(w, tb.lo, tb.lo_len, E & (tb.lo_len - 1));
    const uint32_t eh = E >> tb.lo_bits;
    if (eh != 0) {
        Fr h;
        pb_pl_load(h, tb.hi, tb.hi_len, eh);
        fe_mul(w, w, h);
    }
}
// element i of a row of wire elements (32 bytes each, 16-byte aligned): two 128-bit accesses on the device
KZG_HD void pb_wire_load(Fr& v, const uint32_t* row, size_t i) {
    uint32_t w32[8];
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 a = reinterpret_cast<const uint4*>(row)[2 * i], b = reinterpret_cast<const uint4*>(row)[2 * i + 1];
    w32[0] = a.x; w32[1] = a.y; w32[2] = a.z; w32[3] = a.w; w32[4] = b.x; w32[5] = b.y; w32[6] = b.z; w32[7] = b.w;
#else
    for (int k = 0; k < 8; ++k) w32[k] = row[8 * i + k];
#endif
    fe_from_wire(v, w32);                                  // (-m, 2m)
}
KZG_HD void pb_wire_store(uint32_t* row, size_t i, const Fr& v) {   // v normalised, |v| < 169 m
    uint32_t w32[8];
    fe_to_wire(w32, v);
#if defined(__HIP_DEVICE_COMPILE__)
    reinterpret_cast<uint4*>(row)[2 * i] = make_uint4(w32[0], w32[1], w32[2], w32[3]);
    reinterpret_cast<uint4*>(row)[2 * i + 1] = make_uint4(w32[4], w32[5], w32[6], w32[7]);
#else
    for (int k = 0; k < 8; ++k) row[8 * i + k] = w32[k];
#endif
}

// ---- k_pb_prep: one lane per blob ------------------------------------------------------------------------------------------------------------
// z in (-m, 2m) (pb_wire_load).  Off the domain: the one inversion 1 / (z^n - 1) = 1 / prod_j (z - w^j).  On it (z^n = 1): z / n, the inverse of
// the product without its zero factor -- a product by the constant 1/n, no inversion.
KZG_HD void pb_prep_lane(PbPrep& o, const Fr& z_in, int log_n) {
    Fr z = z_in, zn = z_in, one, den;
    for (int a = 0; a < log_n; ++a) fe_sqr(zn, zn);
    fe_set_one(one);
    fe_sub(den, zn, one);                                  // (-m, 2m) - canonical 1: (-2m, 2m)
    fe_reduce(den);                                        // z^n - 1 in (-m, 2m)
    Fr dc = den;
    fe_canon(dc);
    o.on_domain = fe_is_literal_zero(dc) ? 1u : 0u;
    fe_canon(z);
    Fr inv;
    if (o.on_domain) {
        Fr ninv;
#pragma unroll
        for (int j = 0; j < NL; ++j) ninv.l[j] = (int32_t)FrParams::NINV[log_n * NL + j];
        fe_mul(inv, z, ninv);                              // canonical x canonical constant; z / n in (-m, 2m)
    } else {
        fe_inverse_safegcd(inv, den);
    }
#pragma unroll
    for (int j = 0; j < NL; ++j) { o.z[j] = z.l[j]; o.znm1[j] = den.l[j]; o.tinv[j] = inv.l[j]; }
}

// ---- k_pb_prove: lane t of a blob's workgroup ------------------------------------------------------------------------------------------------
template <int M>
struct PbLane {
    Fr d[M];            // the denominators z - w^j, then their inverses
    Fr pre[M];          // pre[k] = d[0] .. d[k-1] (k >= 1)
    Fr f[M];            // the evaluations f_j (internal form)
    uint32_t zero_k;    // the k of this lane's zero denominator, M when it has none
};

// phase 1 (t < Lf): the M denominators and their product into leaf Lf + t of the tree (NL planes of 2 Lf nodes, heap order: root 1).
// sh = PB_MAX_LOG - log_n: w_n^j = w_4096^(j << sh).
template <int M, class TB>
KZG_HD void pb_lane_denominators(PbLane<M>& lane, int32_t* tree, PbShared* shared, const Fr& z /* canonical */, const TB& tb, uint32_t t, uint32_t Lf, int sh) {
    lane.zero_k = (uint32_t)M;
    Fr p;
#pragma unroll
    for (int k = 0; k < M; ++k) {
        Fr w;
        pb_domain_elem(w, tb, (t + (uint32_t)k * Lf) << sh);
        fe_canon(w);
        fe_sub(lane.d[k], z, w);                           // canonical - canonical: limbs within +-2^29, |d| < m
        if (fe_is_literal_zero(lane.d[k])) {               // z = w^j: 1 stands for the factor, the workgroup learns m = j
            lane.zero_k = (uint32_t)k;
            fe_set_one(lane.d[k]);
            shared->m = t + (uint32_t)k * Lf;
        }
        if (k == 0) p = lane.d[0];
        else { lane.pre[k] = p; fe_mul(p, p, lane.d[k]); }
    }
    pb_pl_store(tree, 2 * Lf, Lf + t, p);
}
// the tree walk of poly_common.h's lds_tree_invert, one node per call.  Up: node = product of its children (callers: s = Lf/2 .. 1, node = s + t, t < s)
KZG_HD void pb_tree_up(int32_t* tree, uint32_t Lf, uint32_t node) {
    const uint32_t S = 2 * Lf;
    Fr a, c, r;
    pb_pl_load(a, tree, S, 2 * node);
    pb_pl_load(c, tree, S, 2 * node + 1);
    fe_mul(r, a, c);
    pb_pl_store(tree, S, node, r);
}
// lane 0: the root's inverse is k_pb_prep's
KZG_HD void pb_tree_root(int32_t* tree, uint32_t Lf, const PbPrep& pr) {
    Fr ri;
#pragma unroll
    for (int j = 0; j < NL; ++j) ri.l[j] = pr.tinv[j];
    pb_pl_store(tree, 2 * Lf, 1, ri);
}
// Down: inverse of a child = inverse of the node x its sibling (callers: s = 1 .. Lf/2, node = s + t, t < s)
KZG_HD void pb_tree_down(int32_t* tree, uint32_t Lf, uint32_t node) {
    const uint32_t S = 2 * Lf;
    Fr g, a, c, ia, ic;
    pb_pl_load(g, tree, S, node);
    pb_pl_load(a, tree, S, 2 * node);
    pb_pl_load(c, tree, S, 2 * node + 1);
    fe_mul2(ia, g, c, ic, g, a);
    pb_pl_store(tree, S, 2 * node, ia);
    pb_pl_store(tree, S, 2 * node + 1, ic);
}
// phase 2 (t < Lf), after the walk: the M inverses (into lane.d), the M evaluations (into lane.f) and, off the domain, the lane's part
// sum_k f_j w^j / (z - w^j) of the barycentric sum (reduced, (-m, 2m)).  On the domain the lane that owns m publishes y = f_m.
template <int M, class TB>
KZG_HD void pb_lane_terms(PbLane<M>& lane, Fr& sum, const int32_t* tree, PbShared* shared, const uint32_t* row, const TB& tb, uint32_t t, uint32_t Lf, int sh,
                          bool on_domain) {
    Fr inv_all;
    pb_pl_load(inv_all, tree, 2 * Lf, Lf + t);
    fe_set_zero(sum);
#pragma unroll
    for (int k = M - 1; k >= 0; --k) {
        Fr inv;
        if (k > 0) { fe_mul(inv, inv_all, lane.pre[k]); fe_mul(inv_all, inv_all, lane.d[k]); }
        else inv = inv_all;
        lane.d[k] = inv;                                   // 1 / d_k (1 where d_k stood for the zero factor)
        const uint32_t jdx = t + (uint32_t)k * Lf;
        pb_wire_load(lane.f[k], row, jdx);
        if (on_domain) continue;                           // y = f_m: no sum (uniform across the workgroup)
        Fr w, term;
        pb_domain_elem(w, tb, jdx << sh);
        fe_mul(term, lane.f[k], w);
        fe_mul(term, term, inv);
        fe_add(sum, sum, term);                            // <= 8 terms of (-m, 2m), normalised after each
        fe_norm(sum);
    }
    if (on_domain) {
        if (lane.zero_k < (uint32_t)M) {
#pragma unroll
            for (int k = 0; k < M; ++k)
                if ((uint32_t)k == lane.zero_k) {
#pragma unroll
                    for (int j = 0; j < NL; ++j) shared->y[j] = lane.f[k].l[j];   // (-m, 2m)
                }
        }
        return;
    }
    fe_reduce(sum);                                        // |sum| < 16 m
}
// the block sum over W = Lf lanes on NL planes of W words (the dead tree): every lane t < W stores, then for dd = W/2 .. 1 the lanes t < dd add
// their partner's value; lane 0 ends with the sum, reduced.  level counts the steps from 0.
KZG_HD void pb_sum_put(int32_t* planes, uint32_t W, uint32_t t, const Fr& v) { pb_pl_store(planes, W, t, v); }
KZG_HD void pb_sum_step(int32_t* planes, uint32_t W, uint32_t t, uint32_t dd, int level, Fr& v) {
    Fr u;
    pb_pl_load(u, planes, W, t + dd);
    fe_add(v, v, u);
    fe_norm(v);
    if (level % 4 == 3) fe_reduce(v);                      // 16 terms of (-m, 2m) since the last reduction
}
// lane 0, z off the domain: y = (z^n - 1) / n x sum (helpers.rs:529-532) into the shared words
KZG_HD void pb_finish_y(PbShared* shared, Fr sum, const PbPrep& pr, int log_n) {
    fe_reduce(sum);                                        // <= 16 terms of (-m, 2m) since the last reduction
    Fr y, znm1, ninv;
#pragma unroll
    for (int j = 0; j < NL; ++j) { znm1.l[j] = pr.znm1[j]; ninv.l[j] = (int32_t)FrParams::NINV[log_n * NL + j]; }
    fe_mul(y, sum, znm1);
    fe_mul(y, y, ninv);                                    // (-m, 2m)
#pragma unroll
    for (int j = 0; j < NL; ++j) shared->y[j] = y.l[j];
}
// lane 0: y to the caller (canonical wire words)
KZG_HD void pb_store_y(uint32_t* ys_wire, size_t blob, const PbShared* shared) {
    Fr y;
#pragma unroll
    for (int j = 0; j < NL; ++j) y.l[j] = shared->y[j];
    pb_wire_store(ys_wire, blob, y);
}
// phase 3 (t < Lf): the lane's M elements of the quotient row, q_j = (y - f_j) / d_j; on the domain also its part of sum_{j != m} q_j w^j
// (reduced, (-m, 2m)); element m is left to pb_store_q_m.
template <int M, class TB>
KZG_HD void pb_lane_quotient(const PbLane<M>& lane, Fr& sum, const PbShared* shared, uint32_t* qrow, const TB& tb, uint32_t t, uint32_t Lf, int sh, bool on_domain) {
    Fr y;
#pragma unroll
    for (int j = 0; j < NL; ++j) y.l[j] = shared->y[j];
    fe_set_zero(sum);
#pragma unroll
    for (int k = 0; k < M; ++k) {
        if ((uint32_t)k == lane.zero_k) continue;
        const uint32_t jdx = t + (uint32_t)k * Lf;
        Fr g, q;
        fe_sub(g, y, lane.f[k]);                           // (-m, 2m) - (-m, 2m): (-3m, 3m), limbs within +-2^29
        fe_mul(q, g, lane.d[k]);
        pb_wire_store(qrow, jdx, q);
        if (!on_domain) continue;
        Fr w, term;
        pb_domain_elem(w, tb, jdx << sh);
        fe_mul(term, q, w);
        fe_add(sum, sum, term);                            // <= 8 terms of (-m, 2m), normalised after each
        fe_norm(sum);
    }
    if (on_domain) fe_reduce(sum);                         // |sum| < 16 m
}
// lane 0, z = w^m: q_m = -(1/z) sum, 1/z = w^(n-m) (kzg.rs:237-260)
template <class TB>
KZG_HD void pb_store_q_m(uint32_t* qrow, Fr sum, const PbShared* shared, const TB& tb, uint32_t n, int sh) {
    fe_reduce(sum);                                        // <= 16 terms of (-m, 2m) since the last reduction
    const uint32_t m = shared->m;
    Fr zinv, q;
    pb_domain_elem(zinv, tb, ((n - m) & (n - 1)) << sh);
    fe_mul(q, sum, zinv);
    fe_neg(q, q);
    fe_norm(q);
    pb_wire_store(qrow, m, q);
}

}  // namespace kzg
