// host_msm_epilogue.h — what the host does with the O(100) points the last kernel of an MSM launch leaves (msm.hip msm_finish): from
// (plan, points) to the launch's results.  Pure host code over host_curve.h and naf.h; also compiled with g++ by
// tests/hostcheck/epiloguecheck.cpp, which checks every form against sum_b weight(b) V_b.
#pragma once
#include "host_curve.h"
#include "msm_plan.h"

namespace kzg {

// results of one launch: one per MSM of a generic batch, one per polynomial of a batched table-mode launch, else one
inline uint32_t msm_results(const Plan& p) { return !p.tables ? p.batch : p.polys ? p.polys : 1u; }

// sum_b (b+1) V_b = T + sum_j 2^j S_j over the bits j of the 0-based bucket index, for the units [unit_lo, unit_lo + units) of 4 096
// buckets each (one MSM: all of them; batched table mode: the units of one polynomial)
inline kzg_host::Xyzz msm_units_result(const Plan& p, const kzg_host::Xyzz* vals, uint32_t unit_lo, uint32_t units) {
    using kzg_host::Xyzz;
    const uint32_t G1 = p.G1(), G1p = p.G1p();
    Xyzz S[32];
    int nbits = 0;
    Xyzz total;
    if (G1 == 1) {
        for (int j = 0; j < 6; ++j) S[j] = vals[j];
        nbits = 6;
        total = vals[6];
    } else {
        const Xyzz* Y = vals;
        const Xyzz* X2 = vals + 6 * G1p;
        for (int j = 0; j < 6; ++j) {
            Xyzz a = kzg_host::xyzz_inf(), b = kzg_host::xyzz_inf();
            for (uint32_t g = unit_lo; g < unit_lo + units; ++g) { a = kzg_host::xyzz_add(a, Y[j * G1p + g]); b = kzg_host::xyzz_add(b, X2[j * G1p + g]); }
            S[j] = a;
            S[6 + j] = b;
        }
        nbits = 12;
        total = kzg_host::xyzz_inf();
        for (uint32_t g = unit_lo; g < unit_lo + units; ++g) total = kzg_host::xyzz_add(total, X2[6 * G1p + g]);
        for (int i = 0; (1u << i) < units; ++i) {
            Xyzz a = kzg_host::xyzz_inf();
            for (uint32_t g = 0; g < units; ++g) if ((g >> i) & 1u) a = kzg_host::xyzz_add(a, X2[6 * G1p + unit_lo + g]);
            S[nbits++] = a;
        }
    }
    if (p.fused && G1 > 1) {                          // the fused level's group g holds the buckets gp * G1 + g: its six sums are the TOP six index bits,
        Xyzz Sk[32];                                  // the second level's the low log2(G1)
        const int lg = ilog2_floor(G1);
        for (int k = 0; k < 6; ++k) Sk[lg + k] = S[k];
        for (int j = 0; j < lg; ++j) Sk[j] = S[6 + j];
        nbits = lg + 6;
        for (int j = 0; j < nbits; ++j) S[j] = Sk[j];
    }
    if (p.naf) {                                      // the bucket index is the key rotated by six bits (naf.h naf_bucket)
        Xyzz Sk[32];
        for (int t = 0; t < nbits; ++t) Sk[naf_key_bit_of_bucket_bit(t, nbits)] = S[t];
        for (int j = 0; j < nbits; ++j) S[j] = Sk[j];
    }
    Xyzz acc = kzg_host::xyzz_inf();
    for (int j = nbits - 1; j >= 0; --j) { acc = kzg_host::xyzz_dbl(acc); acc = kzg_host::xyzz_add(acc, S[j]); }
    if (p.naf) acc = kzg_host::xyzz_dbl(acc);         // bucket b holds the odd digit 2 b + 1: sum_b (2 b + 1) V_b = 2 sum_b b V_b + T
    return kzg_host::xyzz_add(acc, total);
}

// result k < msm_results(p) of the launch whose n_out points are vals[]
inline kzg_host::Xyzz msm_result(const Plan& p, const kzg_host::Xyzz* vals, uint32_t n_out, uint32_t k) {
    // generic mode: sum_w 2^(c w) S_w, <= 255 doublings + W additions per MSM on the host (~0.1 ms)
    if (!p.tables) return kzg_host::horner_windows(vals + (size_t)k * p.W, p.W, p.c);
    if (p.bitsum) {
        kzg_host::Xyzz acc = vals[0];
        for (uint32_t i = 1; i < n_out; ++i) acc = kzg_host::xyzz_add(acc, vals[i]);
        return acc;
    }
    if (p.polys && p.c == 7) return vals[k];           // batched table mode, 64 buckets per polynomial: k_batch_finish left one commitment each
    if (p.polys) {                                     // batched table mode with whole units per polynomial
        const uint32_t units = (1u << (p.c - 1)) / 4096u;
        return msm_units_result(p, vals, k * units, units);
    }
    return msm_units_result(p, vals, 0, p.G1p());
}

inline void msm_epilogue(const Plan& p, const kzg_host::Xyzz* vals, uint32_t n_out, kzg_host::Xyzz* result) {
    for (uint32_t k = 0; k < msm_results(p); ++k) result[k] = msm_result(p, vals, n_out, k);
}

}  // namespace kzg
