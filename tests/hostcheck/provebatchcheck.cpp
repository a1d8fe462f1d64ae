// tests/hostcheck/provebatchcheck.cpp — TEST-ONLY stand-alone program: the lane functions of the batched prover's kernels (csrc/provebatch_lanes.h:
// k_pb_prep's lane, and what a lane of k_pb_prove does between two barriers), compiled by g++ with -DKZG_BOUND_CHECK (every lazy-reduction bound
// aborts with a KZG_BOUND_CHECK line on stderr) and run as ONE workgroup lane by lane: a barrier of the kernel is the end of a loop over t here, in
// the order provebatch.hip has them.  Run by tests/test_prove_batch_host.py.
//
// argv[1] = a file of 32-bit little-endian words written by the test with big integers:
//   log_n, cases, then the two-level table of the 4096-point domain as the library builds it in shape (64 + 64 elements, w^i and w^(64 i), each the
//   8 words of the integer v 2^261 mod r), then per case: on_domain (0 / 1), m, z (8 words, wire), the row (n x 8 words, wire), the expected y
//   (8 words, wire) and the expected quotient row (n x 8 words, wire).
// For every case: the prep lane's flag, its root inverse against the product it stands for (off the domain 1 / (z^n - 1); on it the product of the
// n - 1 non-zero denominators, which z / n replaces), the published index, y and every q_j word for word.
// Prints "prove batch ok log_n=<l> cases=<c> on_domain=<d>" and exits 0 when every answer is the expected one.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "provebatch_lanes.h"

using namespace kzg;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (++failures <= 20) { fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

struct Tables { const int32_t* lo; const int32_t* hi; uint32_t lo_len, hi_len, lo_bits; };

static bool is_one(Fr v) {
    Fr one;
    fe_set_one(one);
    fe_canon(one);
    fe_canon(v);
    return memcmp(v.l, one.l, sizeof v.l) == 0;
}

template <int M>
static void run_case(const Tables& tb, int log_n, const uint32_t* z_wire, const uint32_t* row, bool want_on_domain, uint32_t want_m, const uint32_t* want_y,
                     const uint32_t* want_q, int case_no) {
    const uint32_t n = 1u << log_n, Lf = n / (uint32_t)M;
    const int sh = PB_MAX_LOG - log_n;
    // k_pb_prep
    Fr z;
    pb_wire_load(z, z_wire, 0);
    PbPrep pr;
    pb_prep_lane(pr, z, log_n);
    EXPECT((pr.on_domain != 0) == want_on_domain, "case %d: on_domain %u", case_no, pr.on_domain);
    Fr zc, tinv, znm1;
    for (int j = 0; j < NL; ++j) { zc.l[j] = pr.z[j]; tinv.l[j] = pr.tinv[j]; znm1.l[j] = pr.znm1[j]; }
    {
        Fr prod, chk;
        if (!pr.on_domain) {
            fe_mul(chk, znm1, tinv);
        } else {                                                   // the product z / n replaces: every denominator but the zero one
            fe_set_one(prod);
            for (uint32_t j = 0; j < n; ++j) {
                Fr w, d;
                pb_domain_elem(w, tb, j << sh);
                fe_canon(w);
                fe_sub(d, zc, w);
                if (fe_is_literal_zero(d)) { EXPECT(j == want_m, "case %d: zero denominator at %u", case_no, j); continue; }
                fe_mul(prod, prod, d);
            }
            fe_mul(chk, prod, tinv);
        }
        EXPECT(is_one(chk), "case %d: the root inverse does not invert the root", case_no);
    }
    // k_pb_prove, one workgroup
    std::vector<PbLane<M>> lanes(Lf);
    std::vector<Fr> sums(Lf);
    std::vector<int32_t> tree((size_t)NL * 2 * Lf, 0);
    std::vector<uint32_t> q((size_t)n * 8, 0xA5A5A5A5u), y(8, 0xA5A5A5A5u);
    PbShared shared;
    memset(&shared, 0, sizeof shared);
    shared.m = PB_NO_INDEX;
    const bool on_domain = pr.on_domain != 0;
    for (uint32_t t = 0; t < Lf; ++t) pb_lane_denominators(lanes[t], tree.data(), &shared, zc, tb, t, Lf, sh);
    for (uint32_t s = Lf >> 1; s >= 1; s >>= 1)
        for (uint32_t t = 0; t < s; ++t) pb_tree_up(tree.data(), Lf, s + t);
    pb_tree_root(tree.data(), Lf, pr);
    for (uint32_t s = 1; s < Lf; s <<= 1)
        for (uint32_t t = 0; t < s; ++t) pb_tree_down(tree.data(), Lf, s + t);
    for (uint32_t t = 0; t < Lf; ++t) pb_lane_terms(lanes[t], sums[t], tree.data(), &shared, row, tb, t, Lf, sh, on_domain);
    auto block_sum = [&]() {
        for (uint32_t t = 0; t < Lf; ++t) pb_sum_put(tree.data(), Lf, t, sums[t]);
        int level = 0;
        for (uint32_t dd = Lf >> 1; dd >= 1; dd >>= 1, ++level)
            for (uint32_t t = 0; t < dd; ++t) { pb_sum_step(tree.data(), Lf, t, dd, level, sums[t]); pb_sum_put(tree.data(), Lf, t, sums[t]); }
    };
    if (!on_domain) {
        block_sum();
        pb_finish_y(&shared, sums[0], pr, log_n);
    }
    EXPECT(on_domain ? shared.m == want_m : shared.m == PB_NO_INDEX, "case %d: published index %u", case_no, shared.m);
    pb_store_y(y.data(), 0, &shared);
    for (uint32_t t = 0; t < Lf; ++t) pb_lane_quotient(lanes[t], sums[t], &shared, q.data(), tb, t, Lf, sh, on_domain);
    if (on_domain) {
        block_sum();
        pb_store_q_m(q.data(), sums[0], &shared, tb, n, sh);
    }
    EXPECT(memcmp(y.data(), want_y, 32) == 0, "case %d: y differs", case_no);
    for (uint32_t j = 0; j < n; ++j)
        EXPECT(memcmp(q.data() + 8 * j, want_q + 8 * j, 32) == 0, "case %d: q[%u] differs", case_no, j);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: provebatchcheck <file of cases>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<uint32_t> data;
    uint32_t buf[4096];
    for (size_t k; (k = fread(buf, 4, 4096, f)) != 0;) data.insert(data.end(), buf, buf + k);
    fclose(f);
    if (data.size() < 2 + 128 * 8) { fprintf(stderr, "short file\n"); return 1; }
    const int log_n = (int)data[0];
    const uint32_t cases = data[1];
    if (log_n < 0 || log_n > PB_MAX_LOG) { fprintf(stderr, "log_n out of range\n"); return 1; }
    const size_t n = (size_t)1 << log_n, per_case = 2 + 8 + n * 8 + 8 + n * 8;
    if (data.size() != 2 + 128 * 8 + cases * per_case) { fprintf(stderr, "file size does not match its header\n"); return 1; }
    std::vector<int32_t> lo(NL * 64), hi(NL * 64);
    for (int i = 0; i < 128; ++i) {
        Fr v;
        fe_unpack(v, data.data() + 2 + 8 * i);
        pb_pl_store(i < 64 ? lo.data() : hi.data(), 64, (size_t)(i & 63), v);
    }
    const Tables tb{lo.data(), hi.data(), 64, 64, 6};
    const uint32_t Lf = (uint32_t)(n < (size_t)PB_THREADS ? n : (size_t)PB_THREADS);
    const int M = (int)(n / Lf);
    uint32_t on = 0;
    for (uint32_t c = 0; c < cases; ++c) {
        const uint32_t* p = data.data() + 2 + 128 * 8 + c * per_case;
        const bool od = p[0] != 0;
        on += od;
        const uint32_t *z = p + 2, *row = z + 8, *y = row + n * 8, *q = y + 8;
        switch (M) {
            case 1: run_case<1>(tb, log_n, z, row, od, p[1], y, q, (int)c); break;
            case 2: run_case<2>(tb, log_n, z, row, od, p[1], y, q, (int)c); break;
            case 4: run_case<4>(tb, log_n, z, row, od, p[1], y, q, (int)c); break;
            default: run_case<8>(tb, log_n, z, row, od, p[1], y, q, (int)c); break;
        }
    }
    if (failures) { fprintf(stderr, "provebatchcheck: %d failures\n", failures); return 1; }
    printf("prove batch ok log_n=%d cases=%u on_domain=%u\n", log_n, cases, on);
    return 0;
}
