// tests/hostcheck/header_batch_sanitize_main.cpp — TEST-ONLY stand-alone program (its own main; built with -fsanitize=address,undefined
// by tests/test_header_batch_sanitize_host.py) over the new host code of batched header verification: the weight transcript of
// host_fiat_shamir.h (count 0, 1, 65, 300: serial and fanned out, an identity among the inputs) and pairings_product_is_one of
// host_pairing.h (1, 4, 5 and 9 pairs, identities skipped; with and without a parallel-for).  Prints "header batch sanitize ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>
#include "host_fiat_shamir.h"

using namespace kzg_host;

static void threads_for(size_t n, const std::function<void(size_t)>& job) {
    std::vector<std::thread> ts;
    for (size_t i = 0; i < n; ++i) ts.emplace_back([&job, i] { job(i); });
    for (auto& t : ts) t.join();
}
static void serial_for(size_t n, const std::function<void(size_t)>& job) { for (size_t i = 0; i < n; ++i) job(i); }

static int check_weights(size_t count) {
    const size_t n_shifts = 3;
    std::vector<uint64_t> c(8 * count + 8), c2(16 * count + 16), pi2(16 * count + 16), lens(count + 1), sl = {1, 4, 1024}, sp(8 * n_shifts);
    for (size_t i = 0; i < count; ++i) {
        const uint64_t k[4] = {i + 2, 0, i, 0};
        g1_to_wire(g1_mul_generator(k), c.data() + 8 * i);
        g2_to_wire(g2_mul_generator(k), c2.data() + 16 * i);
        const uint64_t k2[4] = {3 * i + 1, i, 0, 0};
        g2_to_wire(g2_mul_generator(k2), pi2.data() + 16 * i);
        lens[i] = sl[i % 3];
    }
    if (count > 1) memset(c2.data() + 16, 0, 128);                  // an identity
    for (size_t g = 0; g < n_shifts; ++g) { const uint64_t k[4] = {g + 7, 0, 0, 0}; g1_to_wire(g1_mul_generator(k), sp.data() + 8 * g); }
    std::vector<uint64_t> a(4 * (count + 1)), b(4 * (count + 1));
    header_batch_weights_host(c.data(), c2.data(), pi2.data(), lens.data(), count, sl.data(), sp.data(), n_shifts, a.data(), serial_for);
    header_batch_weights_host(c.data(), c2.data(), pi2.data(), lens.data(), count, sl.data(), sp.data(), n_shifts, b.data(), threads_for);
    if (a != b) return 1;
    for (size_t i = 0; i <= count; ++i) {
        uint64_t k[4];
        fr_wire_to_canonical(a.data() + 4 * i, k);
        if (k[2] | k[3]) return 2;                                  // below 2^128
    }
    return 0;
}

static int check_product(int count) {
    // ([a_k]G1, [b_k]G2) with a_k b_k summing to zero: pairs (a, 1), (-a, 1) in turn, the odd one out an identity
    std::vector<G1> ps;
    std::vector<G2> qs;
    const uint64_t one[4] = {1, 0, 0, 0};
    for (int k = 0; k + 1 < count; k += 2) {
        const uint64_t a[4] = {(uint64_t)(5 + k), 9, 0, 0};
        const G1 p = g1_mul_generator(a);
        ps.push_back(p); qs.push_back(g2_mul_generator(one));
        ps.push_back(g1_neg(p)); qs.push_back(g2_mul_generator(one));
    }
    if (count & 1) { ps.push_back(g1_mul_generator(one)); qs.push_back(g2_inf()); }
    if (!pairings_product_is_one(ps.data(), qs.data(), (int)ps.size())) return 3;
    if (!pairings_product_is_one(ps.data(), qs.data(), (int)ps.size(), threads_for)) return 4;
    if (count >= 2) {
        const uint64_t two[4] = {2, 0, 0, 0};
        qs[1] = g2_mul_generator(two);
        if (pairings_product_is_one(ps.data(), qs.data(), (int)ps.size())) return 5;
        if (pairings_product_is_one(ps.data(), qs.data(), (int)ps.size(), threads_for)) return 6;
    }
    return 0;
}

int main() {
    for (size_t count : {(size_t)0, (size_t)1, (size_t)65, (size_t)300}) { const int rc = check_weights(count); if (rc) { printf("weights %zu: %d\n", count, rc); return 1; } }
    for (int count : {0, 1, 4, 5, 9}) { const int rc = check_product(count); if (rc) { printf("product %d: %d\n", count, rc); return 1; } }
    printf("header batch sanitize ok\n");
    return 0;
}
