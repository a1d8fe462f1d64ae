// host_coset_verify.h — the host scalars of the coset-proof batch equation (capi_coset.hip): from the weights r_i, the coset indices k_i and the
// commitment rows c_i of N items, the shifted weights r_i w^(k_i l) and the row sums R_row = sum_{c_i = row} r_i, in the order of the bases
// proofs | proofs | commitments.  Wire form in and out.  Pure host code (no HIP, no engine.h): also compiled alone by g++
// (tests/hostcheck/cosetscalarcheck.cpp).  parallel_for(n, job) runs job(i) for i < n on any threads (the library: kzg::host_parallel_for).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>
#include "host_fr.h"

namespace kzg_host {

// out[i] = r_i w^(k_i l) for the N items, k_i < m = n / l (w^l = w_m from a two-level power table); chunks on the host pool
template <class ParallelFor> void coset_shifted_weights(const uint64_t* coset_indices, const uint64_t* r_powers, size_t N, size_t m, uint64_t* out, ParallelFor parallel_for) {
    const int log_m = __builtin_ctzll(m), lo_bits = (log_m + 1) / 2, hi_bits = log_m - lo_bits;
    const uint64_t* wm = fr_roots().w[log_m];
    std::vector<uint64_t> lo(4 << lo_bits), hi(4 << hi_bits);
    fr_one(lo.data());
    for (size_t j = 1; j < ((size_t)1 << lo_bits); ++j) fr_mul(lo.data() + 4 * (j - 1), wm, lo.data() + 4 * j);
    uint64_t step[4];
    fr_mul(lo.data() + 4 * (((size_t)1 << lo_bits) - 1), wm, step);                  // w_m^(2^lo_bits)
    memcpy(hi.data(), lo.data(), 32);
    for (size_t j = 1; j < ((size_t)1 << hi_bits); ++j) fr_mul(hi.data() + 4 * (j - 1), step, hi.data() + 4 * j);
    const size_t chunks = N >= 1024 ? 32 : 1, per = (N + chunks - 1) / chunks;
    parallel_for(chunks, [&](size_t c) {
        for (size_t i = c * per; i < std::min(N, (c + 1) * per); ++i) {
            const uint64_t k = coset_indices[i];
            uint64_t h[4];
            fr_mul(lo.data() + 4 * (k & (((uint64_t)1 << lo_bits) - 1)), hi.data() + 4 * (k >> lo_bits), h);
            fr_mul(r_powers + 4 * i, h, out + 4 * i);
        }
    });
}

// out = r_i (N) | r_i w^(k_i l) (N) | R_row (M): 2 N + M scalars, every commitment_indices[i] < M
template <class ParallelFor> void coset_batch_scalars(const uint64_t* coset_indices, const uint64_t* commitment_indices, const uint64_t* r_powers, size_t N, size_t M,
                                                      size_t m, uint64_t* out, ParallelFor parallel_for) {
    memcpy(out, r_powers, N * 32);
    coset_shifted_weights(coset_indices, r_powers, N, m, out + 4 * N, parallel_for);
    uint64_t* row_w = out + 8 * N;
    memset(row_w, 0, M * 32);
    for (size_t i = 0; i < N; ++i) { uint64_t* rw = row_w + 4 * commitment_indices[i]; fr_add(rw, r_powers + 4 * i, rw); }
}

// The scalars of a batch of MIXED shapes (kzg_verify_multiproof_batch_mixed): class s has m_s = n_s / l_s cosets, item i the class s_i and k_i < m_{s_i}.
// out = r_{p_j} (N) | r_{p_j} w_{s}^(k l_s) (N) | R_row (M) with p = perm, the order in which the bases hold the proofs (sorted by chunk length) in
// both of their copies.  w_s^(k l_s) = w_{m_s}^k = w_mmax^(k mmax / m_s) with mmax the largest m_s: ONE two-level power table serves every class.
template <class ParallelFor> void coset_batch_scalars_mixed(const uint64_t* class_m, size_t n_classes, const uint64_t* class_indices, const uint64_t* coset_indices,
                                                            const uint64_t* commitment_indices, const uint64_t* r_powers, const uint32_t* perm, size_t N, size_t M,
                                                            uint64_t* out, ParallelFor parallel_for) {
    int log_mmax = 1;
    for (size_t s = 0; s < n_classes; ++s) log_mmax = std::max(log_mmax, (int)__builtin_ctzll(class_m[s]));
    const int lo_bits = (log_mmax + 1) / 2, hi_bits = log_mmax - lo_bits;
    const uint64_t* wm = fr_roots().w[log_mmax];
    std::vector<uint64_t> lo(4 << lo_bits), hi(4 << hi_bits);
    fr_one(lo.data());
    for (size_t j = 1; j < ((size_t)1 << lo_bits); ++j) fr_mul(lo.data() + 4 * (j - 1), wm, lo.data() + 4 * j);
    uint64_t step[4];
    fr_mul(lo.data() + 4 * (((size_t)1 << lo_bits) - 1), wm, step);                  // w_mmax^(2^lo_bits)
    memcpy(hi.data(), lo.data(), 32);
    for (size_t j = 1; j < ((size_t)1 << hi_bits); ++j) fr_mul(hi.data() + 4 * (j - 1), step, hi.data() + 4 * j);
    const size_t chunks = N >= 1024 ? 32 : 1, per = (N + chunks - 1) / chunks;
    parallel_for(chunks, [&](size_t c) {
        for (size_t j = c * per; j < std::min(N, (c + 1) * per); ++j) {
            const size_t i = perm[j];
            const uint64_t e = coset_indices[i] << (log_mmax - (int)__builtin_ctzll(class_m[class_indices[i]]));   // < mmax
            uint64_t h[4];
            fr_mul(lo.data() + 4 * (e & (((uint64_t)1 << lo_bits) - 1)), hi.data() + 4 * (e >> lo_bits), h);
            memcpy(out + 4 * j, r_powers + 4 * i, 32);
            fr_mul(r_powers + 4 * i, h, out + 4 * (N + j));
        }
    });
    uint64_t* row_w = out + 8 * N;
    memset(row_w, 0, M * 32);
    for (size_t i = 0; i < N; ++i) { uint64_t* rw = row_w + 4 * commitment_indices[i]; fr_add(rw, r_powers + 4 * i, rw); }
}

}  // namespace kzg_host
