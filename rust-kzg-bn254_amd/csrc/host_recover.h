// host_recover.h — the host side of kzg_recover_from_cosets (recover.hip, capi_verify.hip): every argument check of the entry, in the
// order the header documents, and what the kernels need from the coset indices -- the sorted list of the MISSING cosets (the roots of
// the vanishing polynomial) and, per coset, the item that carries its values.  Nothing here grows with n: the work is O(m), m = n / l.
// Pure host code: no HIP type, no kzg_ctx, no device call; also compiled with g++ by tests/hostcheck/recovercheck.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/kzg_bn254_mi355x.h"

namespace kzg {

constexpr size_t RECOVER_MAX_N = (size_t)1 << 24;
// The vanishing values are direct products: 2 m |M| field products for |M| missing cosets.  m |M| <= 2^32 admits every (n, l) with
// m <= 2^16 whatever is missing (2^33 products, a few tens of milliseconds) and larger m with proportionally fewer missing cosets.
constexpr uint64_t RECOVER_MAX_PRODUCTS = (uint64_t)1 << 32;
constexpr uint32_t RECOVER_NO_ITEM = 0xFFFFFFFFu;

struct RecoverPlan {
    size_t n = 0, l = 0, m = 0, count = 0;
    int log_n = 0, log_l = 0, log_m = 0;
    size_t degree_bound = 0;               // resolved: 0 of the caller -> count l
    std::vector<uint32_t> missing;         // the cosets without an item, ascending: m - count entries
    std::vector<uint32_t> item_of;         // [coset] -> its item, RECOVER_NO_ITEM for a missing coset: m entries
};

// The checks 2 .. 8 of the header's table (1, the null pointers, is `any_null`), then the plan.  On an error the plan is left empty.
inline int32_t recover_plan(bool any_null, const uint64_t* coset_indices, size_t count, size_t n, size_t chunk_len, size_t degree_bound,
                            RecoverPlan* plan) {
    *plan = RecoverPlan();
    if (any_null) return KZG_ERR_INVALID_ARG;
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_NOT_POWER_OF_TWO;
    if (n > RECOVER_MAX_N) return KZG_ERR_DOMAIN;
    const size_t l = chunk_len;
    if (n == 1 || l == 0 || (l & (l - 1)) != 0 || l > n / 2) return KZG_ERR_INVALID_ARG;
    const size_t m = n / l;
    if (count == 0 || count > m) return KZG_ERR_INVALID_ARG;
    std::vector<uint64_t> seen((m + 63) / 64, 0);                    // one bit per coset: 256 KiB at m = 2^24
    for (size_t i = 0; i < count; ++i) {
        const uint64_t k = coset_indices[i];
        if (k >= m) return KZG_ERR_INVALID_ARG;
        uint64_t& word = seen[k >> 6];
        const uint64_t bit = (uint64_t)1 << (k & 63);
        if (word & bit) return KZG_ERR_INVALID_ARG;                  // the same coset twice
        word |= bit;
    }
    if (degree_bound > count * l) return KZG_ERR_INVALID_ARG;        // too few cosets for that degree
    if ((uint64_t)m * (uint64_t)(m - count) > RECOVER_MAX_PRODUCTS) return KZG_ERR_TOO_LARGE;
    plan->n = n; plan->l = l; plan->m = m; plan->count = count;
    plan->log_n = __builtin_ctzll(n); plan->log_l = __builtin_ctzll(l); plan->log_m = plan->log_n - plan->log_l;
    plan->degree_bound = degree_bound ? degree_bound : count * l;
    plan->item_of.assign(m, RECOVER_NO_ITEM);
    for (size_t i = 0; i < count; ++i) plan->item_of[coset_indices[i]] = (uint32_t)i;
    plan->missing.reserve(m - count);
    for (size_t k = 0; k < m; ++k)
        if (plan->item_of[k] == RECOVER_NO_ITEM) plan->missing.push_back((uint32_t)k);
    return KZG_OK;
}

}  // namespace kzg
