// tests/hostcheck/proof_scalars.cpp — TEST-ONLY driver for a plain g++ build of csrc/proof_plan.h proof_fill_scalars: the chain's scalar table at
// five points z (7, off every domain; 1; w; w^(n-1); 0) on six domain sizes, and at z = 1 on every size from 2 to 4096 (the table behind the
// known-index form), one line per case: log_n, the point's name, whether z came out on the domain, then the 2 log n + 6 elements as 256-bit hex
// numbers (wire form).  tests/test_proof_scalars_host.py compares them with big integers; also run under ASan + UBSan (tests/test_sanitizers_host.py).
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "proof_plan.h"

using namespace kzg;

static void run(int log_n, const char* name, const uint64_t z[4]) {
    // exactly the table's size, on the heap: a write past zt_count elements is an error under ASan
    uint64_t* zt = new uint64_t[(size_t)ProofStaging::zt_count(log_n) * 4];
    bool on = false;
    proof_fill_scalars(z, log_n, zt, &on);
    printf("%d %s %d", log_n, name, (int)on);
    for (int i = 0; i < ProofStaging::zt_count(log_n); ++i)
        printf(" %016llx%016llx%016llx%016llx", (unsigned long long)zt[4 * i + 3], (unsigned long long)zt[4 * i + 2], (unsigned long long)zt[4 * i + 1], (unsigned long long)zt[4 * i]);
    printf("\n");
    delete[] zt;
}

int main() {
    const uint64_t seven_int[4] = {7, 0, 0, 0}, zero[4] = {0, 0, 0, 0};
    uint64_t seven[4], one[4];
    kzg_host::fr_mul(kzg_host::FR_R2, seven_int, seven);
    kzg_host::fr_one(one);
    for (int log_n : {0, 1, 9, 12, 20, 28}) {
        run(log_n, "off", seven);
        run(log_n, "one", one);
        run(log_n, "w", kzg_host::fr_roots().w[log_n]);
        run(log_n, "w^(n-1)", kzg_host::fr_roots().winv[log_n]);
        run(log_n, "zero", zero);
    }
    for (int log_n = 1; log_n <= PROOF_SMALL_MAX_LOG; ++log_n) run(log_n, "z1", one);
    return 0;
}
