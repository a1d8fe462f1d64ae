// tests/hostcheck/cosetscalarcheck.cpp — TEST-ONLY driver for a plain g++ build of csrc/host_coset_verify.h (no GPU, no library): the host scalars
// of the coset-proof batch equation, r_i | r_i w^(k_i l) | row sums, on inputs both sides can write down.  Item i has the weight with the canonical
// words {a, ~a, 3 a, i & 0xffff}, a = (i + 1) 0x9e3779b97f4a7c15 mod 2^64; its coset index is 0 (kmode 0), m - 1 (kmode 1) or cycles through
// 0, m - 1, (2654435761 i + 3) mod m (kmode 2); its row is M - 1 (cmode 0: every item on one row) or i mod M (cmode 1).  One line per case:
// log_m N M kmode cmode, then the 2 N + M scalars as 256-bit hex numbers (wire form).  The chunks run on threads of their own, as they do on the
// library's pool.  tests/test_coset_scalars_host.py compares with big integers and also builds this file with ASan + UBSan.
#include <cstdio>
#include <functional>
#include <thread>
#include <vector>

#include "host_coset_verify.h"

static void threads_for(size_t n, const std::function<void(size_t)>& job) {
    std::vector<std::thread> ts;
    for (size_t i = 1; i < n; ++i) ts.emplace_back([&job, i] { job(i); });
    if (n) job(0);
    for (auto& t : ts) t.join();
}

static void run(int log_m, size_t N, size_t M, int kmode, int cmode) {
    const uint64_t m = (uint64_t)1 << log_m;
    // exactly the sizes the header is told, on the heap: a read or write past them is an error under ASan
    std::vector<uint64_t> r(4 * N), ks(N), cs(N), out(4 * (2 * N + M), 0xdeadbeefULL);
    for (size_t i = 0; i < N; ++i) {
        const uint64_t a = (uint64_t)(i + 1) * 0x9e3779b97f4a7c15ULL, x[4] = {a, ~a, 3 * a, (uint64_t)(i & 0xffff)};
        kzg_host::fr_mul(kzg_host::FR_R2, x, r.data() + 4 * i);
        ks[i] = kmode == 0 ? 0 : kmode == 1 ? m - 1 : i % 3 == 0 ? 0 : i % 3 == 1 ? m - 1 : (2654435761ULL * i + 3) % m;
        cs[i] = cmode == 0 ? M - 1 : i % M;
    }
    kzg_host::coset_batch_scalars(ks.data(), cs.data(), r.data(), N, M, (size_t)m, out.data(), threads_for);
    printf("%d %zu %zu %d %d", log_m, N, M, kmode, cmode);
    for (size_t i = 0; i < 2 * N + M; ++i)
        printf(" %016llx%016llx%016llx%016llx", (unsigned long long)out[4 * i + 3], (unsigned long long)out[4 * i + 2], (unsigned long long)out[4 * i + 1], (unsigned long long)out[4 * i]);
    printf("\n");
}

int main() {
    run(1, 1, 1, 2, 1);            // m = 2: the high table has one entry
    run(1, 1025, 3, 2, 1);
    run(5, 1023, 4, 2, 1);         // odd log m; one chunk
    run(6, 1024, 4, 2, 1);         // even log m; 32 chunks of 32
    run(6, 1025, 2000, 2, 1);      // 32 chunks of 33, the last one short; M > N: rows of weight zero
    run(5, 7, 12, 0, 1);           // every coset index 0
    run(5, 7, 3, 1, 0);            // every coset index m - 1, every item on the last row
    run(6, 1, 5, 1, 0);
    run(23, 1030, 2, 2, 1);        // a large domain of cosets: 2^12 + 2^11 table entries
    return 0;
}
