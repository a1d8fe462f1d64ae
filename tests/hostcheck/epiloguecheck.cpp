// tests/hostcheck/epiloguecheck.cpp — TEST-ONLY driver for a plain g++ build (no GPU, no library) of csrc/host_msm_epilogue.h: the host
// epilogue of every MSM form against the definition.  Bucket values V = k G with small known k; the points a launch would leave are built
// from the kernels' definitions (msm_kernels.h sections 6b / 6c: bit-plane sums per group of 64 buckets, k_red_bits2*: the same over the
// group totals, k_batch_finish, the fused level's strided groups, naf.h naf_bucket); the epilogue's result must be (sum weight k) G, with
// weight = bucket + 1 for fixed windows and 2 key + 1 for NAF digits.  Two draws per shape: random k, and k with identities and many equal
// buckets.  The plans come from make_plan, so the shapes are real ones.  Prints "epiloguecheck ok"; built and run by
// tests/test_msm_plan_host.py and, under ASan + UBSan, by tests/test_sanitizers_host.py.
#include <cstdio>
#include <functional>
#include <vector>

#include "host_msm_epilogue.h"

using namespace kzg;
using kzg_host::Xyzz;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "epiloguecheck: check failed: %s (line %d, %s)\n", #c, __LINE__, what); return false; } } while (0)

static Xyzz KG[256];                                   // k G, k < 256 (k = 0: the identity)
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }
// draw 0: 1 .. 255; draw 1: a quarter identities, the rest 1 .. 3 (equal buckets next to each other: the doubling case of every addition)
static uint32_t draw_k(int draw) { return draw == 0 ? 1 + rnd() % 255 : (rnd() & 3) == 0 ? 0 : 1 + rnd() % 3; }

// N G for a 320-bit N (5 words, low first), by double-and-add: (N mod r) G without reducing N
struct Big { uint64_t w[5] = {}; };
static void big_shl(Big& a, int c) { for (int i = 4; i >= 0; --i) a.w[i] = (a.w[i] << c) | (i ? a.w[i - 1] >> (64 - c) : 0); }
static void big_add(Big& a, uint64_t v) { for (int i = 0; i < 5 && v; ++i) { const uint64_t s = a.w[i] + v; v = s < v; a.w[i] = s; } }
static Xyzz big_mul_g(const Big& n) {
    Xyzz acc = kzg_host::xyzz_inf();
    for (int i = 319; i >= 0; --i) {
        acc = kzg_host::xyzz_dbl(acc);
        if ((n.w[i / 64] >> (i % 64)) & 1) acc = kzg_host::xyzz_add(acc, KG[1]);
    }
    return acc;
}
static bool same_point(const Xyzz& a, const Xyzz& b) {
    uint64_t xa[8], xb[8];
    uint8_t ia = 0, ib = 0;
    kzg_host::xyzz_to_affine(a, xa, &ia);
    kzg_host::xyzz_to_affine(b, xb, &ib);
    return ia == ib && memcmp(xa, xb, 64) == 0;
}
static void add_to(Xyzz& a, const Xyzz& b) { a = kzg_host::xyzz_add(a, b); }

// The result points of a table-mode launch over the bucket array k[] (k[pos] G at position pos < B), level by level
static std::vector<Xyzz> table_mode_points(const Plan& p, const std::vector<uint32_t>& k) {
    const uint32_t G1 = p.G1(), G1p = p.G1p();
    // level 1: X1[role][g], role j < 6 = sum over the group's values whose index has bit j, role 6 = their total; the group's value gp is
    // bucket 64 g + gp, or (fused level) bucket gp G1 + g
    std::vector<Xyzz> x1((size_t)7 * G1, kzg_host::xyzz_inf());
    for (uint32_t g = 0; g < G1; ++g)
        for (uint32_t gp = 0; gp < 64; ++gp) {
            const Xyzz& v = KG[k[p.fused ? gp * G1 + g : g * 64 + gp]];
            for (int j = 0; j < 6; ++j) if ((gp >> j) & 1u) add_to(x1[(size_t)j * G1 + g], v);
            add_to(x1[(size_t)6 * G1 + g], v);
        }
    std::vector<Xyzz> out;
    if (p.polys && p.c == 7) {                           // k_batch_finish: 2 sum_j 2^j S_j + T per group
        for (uint32_t g = 0; g < p.polys; ++g) {
            Xyzz acc = x1[(size_t)5 * G1 + g];
            for (int j = 4; j >= -1; --j) acc = kzg_host::xyzz_add(kzg_host::xyzz_dbl(acc), x1[(size_t)(j >= 0 ? j : 6) * G1 + g]);
            out.push_back(acc);
        }
    } else if (G1 == 1) {
        out = x1;
    } else {                                             // level 2: out[a G1p + g'] = sum of X1[a][64 g' ..), then the bit-plane sums of the totals X1[6]
        out.assign((size_t)13 * G1p, kzg_host::xyzz_inf());
        for (uint32_t a = 0; a < 6; ++a)
            for (uint32_t g = 0; g < G1; ++g) add_to(out[(size_t)a * G1p + g / 64], x1[(size_t)a * G1 + g]);
        for (uint32_t g = 0; g < G1; ++g) {
            const Xyzz& v = x1[(size_t)6 * G1 + g];
            for (int j = 0; j < 6; ++j) if (((g % 64) >> j) & 1u) add_to(out[(size_t)6 * G1p + (size_t)j * G1p + g / 64], v);
            add_to(out[(size_t)6 * G1p + (size_t)6 * G1p + g / 64], v);
        }
    }
    return out;
}

static PlanContext alone_ctx(int c_override = 0) { PlanContext c; c.msm_c_override = c_override; return c; }
static MsmBasesShape tables(int c, bool naf = false) {
    MsmBasesShape b;
    b.table_stride = 1u << 20; b.c = c; b.W = naf ? 255 : (255 + c - 1) / c; b.naf = naf;
    return b;
}

// one table-mode shape: `results` sums over `per` keys each; key -> position of its bucket in the array
static bool check_tables(const char* what, const Plan& p, uint32_t results, uint32_t per, const std::function<uint32_t(uint32_t r, uint32_t key)>& pos) {
    CHECK(p.tables && !p.bitsum && msm_results(p) == results);
    for (int draw = 0; draw < 2; ++draw) {
        std::vector<uint32_t> k(p.B, 0);
        std::vector<uint64_t> want(results, 0);
        for (uint32_t r = 0; r < results; ++r)
            for (uint32_t key = 0; key < per; ++key) {
                const uint32_t kb = draw_k(draw);
                CHECK(pos(r, key) < p.B && k[pos(r, key)] == 0);
                k[pos(r, key)] = kb;
                want[r] += (uint64_t)(p.naf ? 2 * key + 1 : key + 1) * kb;
            }
        const std::vector<Xyzz> vals = table_mode_points(p, k);
        CHECK(vals.size() == p.n_out);
        std::vector<Xyzz> got(results);
        msm_epilogue(p, vals.data(), p.n_out, got.data());
        for (uint32_t r = 0; r < results; ++r) {
            Big n;
            n.w[0] = want[r];
            CHECK(same_point(got[r], big_mul_g(n)));
        }
    }
    return true;
}

// generic mode: W window sums per MSM, S_w = sum_b (b + 1) V_b over 2^(c-1) buckets (running sum), Horner on the host
static bool check_generic(const char* what, int c, uint32_t batch) {
    const Plan p = make_plan(alone_ctx(c), 100, MsmBasesShape{}, batch);
    CHECK(!p.tables && p.c == c && p.batch == batch && msm_results(p) == batch && p.n_out == (uint32_t)p.W * batch);
    for (int draw = 0; draw < 2; ++draw) {
        std::vector<Xyzz> vals(p.n_out);
        std::vector<Big> want(batch);
        for (uint32_t m = 0; m < batch; ++m) {
            std::vector<uint64_t> s(p.W, 0);
            for (int w = 0; w < p.W; ++w) {
                Xyzz run = kzg_host::xyzz_inf(), sum = kzg_host::xyzz_inf();
                for (uint32_t b = p.B; b-- > 0;) {
                    const uint32_t kb = draw_k(draw);
                    add_to(run, KG[kb]);
                    add_to(sum, run);
                    s[w] += (uint64_t)(b + 1) * kb;
                }
                vals[(size_t)m * p.W + w] = sum;
            }
            for (int w = p.W - 1; w >= 0; --w) { big_shl(want[m], c); big_add(want[m], s[w]); }
        }
        std::vector<Xyzz> got(batch);
        msm_epilogue(p, vals.data(), p.n_out, got.data());
        for (uint32_t m = 0; m < batch; ++m) CHECK(same_point(got[m], big_mul_g(want[m])));
    }
    return true;
}

static bool check_bitsum(const char* what, size_t n, uint32_t points) {
    MsmBasesShape b;
    b.table_stride = 1u << 15; b.W = 255; b.bitsum = true;
    const Plan p = make_plan(alone_ctx(), n, b, 1);
    CHECK(p.bitsum && p.n_out == points && msm_results(p) == 1);
    for (int draw = 0; draw < 2; ++draw) {
        std::vector<Xyzz> vals(points);
        Big want;
        for (auto& v : vals) { const uint32_t kb = draw_k(draw); v = KG[kb]; big_add(want, kb); }
        Xyzz got;
        msm_epilogue(p, vals.data(), p.n_out, &got);
        CHECK(same_point(got, big_mul_g(want)));
    }
    return true;
}

int main() {
    KG[0] = kzg_host::xyzz_inf();
    KG[1].x = kzg_host::FQ_ONE; KG[1].y = kzg_host::dbl(kzg_host::FQ_ONE); KG[1].zz = kzg_host::FQ_ONE; KG[1].zzz = kzg_host::FQ_ONE;     // G = (1, 2)
    for (int i = 2; i < 256; ++i) KG[i] = kzg_host::xyzz_add(KG[i - 1], KG[1]);
    bool ok = true;
    const auto plain = [](uint32_t, uint32_t key) { return key; };
    {   // one group of 64 buckets: its seven sums are the result points
        const Plan p = make_plan(alone_ctx(), 1000, tables(7), 1);
        ok &= p.B == 64 && p.G1() == 1 && check_tables("B = 64", p, 1, 64, plain);
    }
    {   // two units of 4 096 buckets, accumulated and fused
        const Plan p = make_plan(alone_ctx(), 2048, tables(14), 1), f = make_plan(alone_ctx(), 512, tables(14), 1);
        ok &= p.B == 8192 && p.G1p() == 2 && !p.fused && check_tables("B = 8192", p, 1, 8192, plain);
        ok &= f.B == 8192 && f.fused && check_tables("B = 8192 fused", f, 1, 8192, plain);
    }
    for (int c : {13, 17}) {   // NAF digits: bucket = the key rotated by six bits
        const Plan p = make_plan(alone_ctx(), c == 13 ? (size_t)1 << 14 : (size_t)1 << 20, tables(c, true), 1);
        ok &= p.naf && p.c == c && p.B == 1u << (c - 1) && check_tables(c == 13 ? "NAF B = 4096" : "NAF B = 65536", p, 1, p.B, [&](uint32_t, uint32_t key) { return naf_bucket(key, c - 1); });
    }
    {   // batched: whole units per polynomial (one, four), and 64 buckets per polynomial (finished on the device: passed through)
        const Plan p13 = make_plan(alone_ctx(), (size_t)3 << 13, tables(13, true), 1, 3), p15 = make_plan(alone_ctx(), (size_t)2 << 15, tables(15, true), 1, 2),
                   p7 = make_plan(alone_ctx(), 3 * 64, tables(13, true), 1, 3);
        ok &= p13.polys == 3 && p13.c == 13 && p13.G1p() == 3 &&
              check_tables("polys = 3, c = 13", p13, 3, 4096, [](uint32_t r, uint32_t key) { return (r << 12) | naf_bucket(key, 12); });
        ok &= p15.polys == 2 && p15.c == 15 && p15.G1p() == 8 &&
              check_tables("polys = 2, c = 15", p15, 2, 16384, [](uint32_t r, uint32_t key) { return (r << 14) | naf_bucket(key, 14); });
        ok &= p7.polys == 3 && p7.c == 7 && p7.B == 256 && check_tables("polys = 3, c = 7", p7, 3, 64, [](uint32_t r, uint32_t key) { return (r << 6) | key; });
    }
    for (int c : {4, 13})
        for (uint32_t batch : {1u, 3u}) ok &= check_generic(c == 4 ? "generic c = 4" : "generic c = 13", c, batch);
    ok &= check_bitsum("bit sums, 1 point", 1, 1) && check_bitsum("bit sums, 8 points", 4096, 8);
    if (ok) printf("epiloguecheck ok\n");
    return ok ? 0 : 1;
}
