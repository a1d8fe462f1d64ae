// tests/hostcheck/provecosetscheck.cpp — TEST-ONLY driver for a plain g++ build (no GPU, no library) of the host side of kzg_prove_cosets
// (csrc/host_prove_cosets.h).  It checks
//   1. the argument table: the shape checks in the encoder's order behind the pointers and count = 0, the items with the smallest bad one,
//      the overflowing sizes last;
//   2. group sizes monotone in the budget, never 0, never above the items, the groups covering the items;
//   3. the bytes of an item against the highest index each launch of the driver addresses (the addressing of provecosets.hip restated in
//      the model below, on buffers of exactly the planned sizes with checked access);
//   4. S, the segments and the levels of every shape of a grid, and that no lane runs more than S dependent products in a pass;
//   5. a host model of the three passes -- the index arithmetic of the kernels (pc_* of the header), the arithmetic of host_fr.h -- against
//      the sequential recurrence and the identity f = q (X^l - c) + r, for a grid of (d, l, S, k) that reaches five levels;
// and prints the plans of a small grid in the format of tests/golden/prove_cosets_plans.txt.  Built and run by
// tests/test_prove_cosets_plan_host.py, plain and under ASan + UBSan.  Exit status 1 and a line on stderr per violated check.
#include <array>
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_fr.h"
#include "host_prove_cosets.h"

using namespace kzg;
using namespace kzg_host;

static int failures = 0;
static char case_name[256] = "";
#define CHECK(c) do { if (!(c)) { ++failures; fprintf(stderr, "provecosetscheck: %s: line %d: %s\n", case_name, __LINE__, #c); } } while (0)

typedef std::array<uint64_t, 4> El;

// ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
static void check_order() {
    snprintf(case_name, sizeof case_name, "order");
    const size_t SRS = 3000;
    CHECK(prove_cosets_check_shape(false, false, 1, 64, 128, 1, SRS) == KZG_OK);
    CHECK(prove_cosets_check_shape(true, true, 0, 3, 0, 0, 0) == KZG_ERR_INVALID_ARG);
    CHECK(prove_cosets_check_shape(false, false, 0, 3, 0, 1, SRS) == KZG_ERR_INVALID_ARG);         // count = 0 in front of a length that is no power of two
    CHECK(prove_cosets_check_shape(false, true, 1, 3, 0, 1, SRS) == KZG_ERR_INVALID_ARG);          // the SRS in front of the lengths
    CHECK(prove_cosets_check_shape(false, false, 1, 0, 64, 1, SRS) == KZG_ERR_NOT_POWER_OF_TWO);
    CHECK(prove_cosets_check_shape(false, false, 1, 48, (size_t)1 << 25, 1, SRS) == KZG_ERR_NOT_POWER_OF_TWO);
    CHECK(prove_cosets_check_shape(false, false, 1, 64, 96, 1, SRS) == KZG_ERR_NOT_POWER_OF_TWO);
    CHECK(prove_cosets_check_shape(false, false, 1, 1, (size_t)1 << 25, 3, SRS) == KZG_ERR_DOMAIN);
    CHECK(prove_cosets_check_shape(false, false, 1, 4096, 2048, 1, SRS) == KZG_ERR_INVALID_ARG);
    CHECK(prove_cosets_check_shape(false, false, 1, 1, 64, 1, SRS) == KZG_ERR_INVALID_ARG);
    CHECK(prove_cosets_check_shape(false, false, 1, 4096, 4096, 3, SRS) == KZG_ERR_INVALID_ARG);
    CHECK(prove_cosets_check_shape(false, false, 1, 64, 4096, 64, SRS) == KZG_ERR_INVALID_ARG);
    CHECK(prove_cosets_check_shape(false, false, 1, 4096, 4096, 1, SRS) == KZG_ERR_SRS_CAPACITY_EXCEEDED);
    CHECK(prove_cosets_check_shape(false, false, 1, 4096, 4096, 1, SIZE_MAX) == KZG_OK);           // no SRS: no row 6
    // every error of encode_check is the error of this check with count = 1
    for (size_t d : {(size_t)0, (size_t)1, (size_t)2, (size_t)48, (size_t)64, (size_t)4096})
        for (size_t n : {(size_t)0, (size_t)64, (size_t)96, (size_t)4096, (size_t)1 << 25})
            for (size_t l : {(size_t)0, (size_t)1, (size_t)3, (size_t)32, (size_t)64})
                CHECK(prove_cosets_check_shape(false, false, 1, d, n, l, SRS) == encode_check(false, false, d, n, l, SRS));
    // the items: the smallest bad one, polynomial or coset; bad may be null
    const uint64_t ks[5] = {0, 31, 32, 7, 99}, ps[5] = {0, 1, 0, 2, 0};
    uint64_t bad = 77;
    CHECK(prove_cosets_check_items(nullptr, ks, 2, 1, 32, &bad) == KZG_OK && bad == 77);
    CHECK(prove_cosets_check_items(nullptr, ks, 5, 1, 32, &bad) == KZG_ERR_INVALID_ARG && bad == 2);
    CHECK(prove_cosets_check_items(ps, ks, 5, 1, 32, &bad) == KZG_ERR_INVALID_ARG && bad == 1);
    CHECK(prove_cosets_check_items(ps, ks, 5, 2, 64, &bad) == KZG_ERR_INVALID_ARG && bad == 3);
    CHECK(prove_cosets_check_items(ps, ks, 5, 3, 64, &bad) == KZG_ERR_INVALID_ARG && bad == 4);
    CHECK(prove_cosets_check_items(ps, ks, 5, 3, 100, &bad) == KZG_OK);
    CHECK(prove_cosets_check_items(ps, ks, 5, 1, 32, nullptr) == KZG_ERR_INVALID_ARG);
    CHECK(prove_cosets_check_items(nullptr, ks, 0, 1, 1, &bad) == KZG_OK);
    // the sizes
    CHECK(prove_cosets_check_sizes(1, 64, 1, 4, false) == KZG_OK);
    CHECK(prove_cosets_check_sizes(SIZE_MAX / (64 * 32), 64, 1, 4, false) == KZG_OK);
    CHECK(prove_cosets_check_sizes(SIZE_MAX / (64 * 32) + 1, 64, 1, 4, false) == KZG_ERR_INVALID_ARG);
    CHECK(prove_cosets_check_sizes(1, 64, 1, SIZE_MAX / 64, false) == KZG_OK);                       // a proof is 64 bytes, a value row 32
    CHECK(prove_cosets_check_sizes(1, 64, 1, SIZE_MAX / 64 + 1, false) == KZG_ERR_INVALID_ARG);
    CHECK(prove_cosets_check_sizes(1, 64, 4, SIZE_MAX / 128 + 1, false) == KZG_ERR_INVALID_ARG);
    CHECK(prove_cosets_check_sizes(1, 64, 1, SIZE_MAX / (64 * 32) + 1, true) == KZG_ERR_INVALID_ARG);  // a quotient row is d x 32 bytes
    CHECK(prove_cosets_check_sizes(1, 64, 1, SIZE_MAX / (64 * 32), true) == KZG_OK);
}

// ---- 2, 4 ------------------------------------------------------------------------------------------------------------------------------
static void check_plan(size_t d, size_t n, size_t l, size_t items, bool values, bool quotients) {
    snprintf(case_name, sizeof case_name, "plan d=%zu n=%zu l=%zu items=%zu v=%d q=%d", d, n, l, items, (int)values, (int)quotients);
    const ProveCosetsPlan p = prove_cosets_plan(d, n, l, items, values, quotients, 0);
    const size_t D = d / l;
    CHECK(p.D == D && p.m == n / l && p.S == std::min<size_t>(D, PROVE_SEG) && ((size_t)1 << p.log_S) == p.S);
    CHECK(p.n_levels >= 1 && p.n_levels <= PROVE_MAX_LEVELS && p.level[p.n_levels - 1].nseg == 1);
    size_t len = D, heads = 0;
    for (int i = 0; i < p.n_levels; ++i) {
        const ProveLevel& L = p.level[i];
        CHECK(L.len == len && L.nseg == (len + p.S - 1) / p.S && L.shift == p.log_l + i * p.log_S);
        CHECK((L.nseg > 1) == (i + 1 < p.n_levels));
        CHECK(L.heads == (i == 0 || L.nseg > 1) && L.heads_off == heads);
        if (i > 0) CHECK(L.data_off == p.level[i - 1].heads_off);
        if (L.heads) heads += (size_t)L.nseg * l;
        CHECK(((size_t)l << (i * p.log_S)) * L.len >= d);                           // the level's multiplier spans the chain: l S^i len >= d
        len = L.nseg;
    }
    CHECK(p.heads_elems == heads);
    CHECK(p.item_bytes >= (quotients ? d * 32 : 0) + heads * 32 + (values ? l * 32 : 0) + PROVE_ITEM_INDEX_BYTES);
    const uint32_t ntt_passes = values && l > 1 ? (uint32_t)((p.log_l + NTT_KMAX - 1) / NTT_KMAX) : 0u;
    CHECK(p.launches == (uint32_t)p.n_levels + (uint32_t)std::max(p.n_levels - 2, 0) + 1u + ntt_passes);  // local passes, fix-ups above level 0, level 0's, the transform
    // groups against the budget
    size_t last = 0;
    std::vector<size_t> budgets = {(size_t)1, p.item_bytes - 1, p.item_bytes, 2 * p.item_bytes - 1, 2 * p.item_bytes, 3 * p.item_bytes + 5, (size_t)1 << 20,
                                   (size_t)1 << 30, (size_t)4 << 30, (size_t)1 << 40};
    std::sort(budgets.begin(), budgets.end());
    for (size_t budget : budgets) {
        const ProveCosetsPlan b = prove_cosets_plan(d, n, l, items, values, quotients, budget);
        CHECK(b.group >= 1 && b.group <= std::max<size_t>(items, 1) && b.group <= PROVE_GROUP_MAX);
        CHECK(b.group >= last);                                                     // monotone in the budget
        CHECK(b.group == 1 || b.group * b.item_bytes <= budget);
        CHECK(b.group == std::max<size_t>(items, 1) || b.group == PROVE_GROUP_MAX || (b.group + 1) * b.item_bytes > budget);
        CHECK(b.n_groups * b.group >= items && (items == 0 ? b.n_groups == 0 : (b.n_groups - 1) * b.group < items));
        CHECK(b.group_bytes == b.group * b.item_bytes && b.item_bytes == p.item_bytes && b.S == p.S && b.n_levels == p.n_levels);
        CHECK(b.msm_single == (b.group <= PROVE_MSM_SINGLE_MAX_ITEMS));
        last = b.group;
    }
}

// ---- 3, 5: the host model ----------------------------------------------------------------------------------------------------------------
struct Buf {                                          // a device buffer of exactly `size` elements: every access is checked
    std::vector<El> v;
    const char* name;
    Buf(size_t size, const char* nm) : v(size), name(nm) { for (auto& e : v) e = {7, 7, 7, 7}; }
    El& at(size_t i) {
        if (i >= v.size()) { ++failures; fprintf(stderr, "provecosetscheck: %s: %s[%zu] is outside its %zu elements\n", case_name, name, i, v.size()); static El dummy; return dummy; }
        return v[i];
    }
};
static El fr_pow_w(int log_n, uint32_t e) {           // w_n^e
    El acc, base;
    fr_one(acc.data());
    memcpy(base.data(), fr_roots().w[log_n], 32);
    for (; e; e >>= 1) {
        if (e & 1) fr_mul(acc.data(), base.data(), acc.data());
        fr_mul(base.data(), base.data(), base.data());
    }
    return acc;
}
static uint32_t max_products = 0;                     // the most dependent products a lane ran in one pass

// k_pc_local: lane x of one item
static void model_local(const ProveCosetsPlan& p, int level, uint32_t k, const std::vector<El>& f, Buf& q, Buf& heads, bool keep) {
    const ProveLevel& L = p.level[level];
    const uint32_t l = (uint32_t)p.l, mask = (uint32_t)(p.n - 1);
    for (uint32_t x = 0; x < L.nseg * l; ++x) {
        const uint32_t rho = x & (l - 1), seg = x >> p.log_l;
        const El c = fr_pow_w(p.log_n, pc_mult_exp(k, L.shift, mask));
        El acc = {0, 0, 0, 0};
        const uint32_t lo = seg << p.log_S, hi = std::min(lo + (1u << p.log_S), L.len);
        uint32_t products = 0;
        for (uint32_t j = hi; j-- > lo;) {
            const El a = level == 0 ? f[pc_elem(j, l, rho)] : heads.at(L.data_off + pc_elem(j, l, rho));
            El t;
            fr_mul(c.data(), acc.data(), t.data());
            ++products;
            fr_add(t.data(), a.data(), acc.data());
            if (level == 0) { if (keep && j > 0) q.at(pc_quot_elem(j, l, rho)) = acc; }
            else heads.at(L.data_off + pc_elem(j, l, rho)) = acc;
        }
        max_products = std::max(max_products, products);
        if (L.heads) heads.at(L.heads_off + pc_elem(seg, l, rho)) = acc;
    }
}
// k_pc_fix
static void model_fix(const ProveCosetsPlan& p, int level, uint32_t k, Buf& heads) {
    const ProveLevel& L = p.level[level];
    const uint32_t l = (uint32_t)p.l, mask = (uint32_t)(p.n - 1);
    for (uint32_t x = 0; x < L.len * l; ++x) {
        const uint32_t rho = x & (l - 1), j = x >> p.log_l, seg = j >> p.log_S;
        if (seg + 1 >= L.nseg) continue;
        const El w = fr_pow_w(p.log_n, pc_pow_exp(k, L.shift, ((seg + 1) << p.log_S) - j, mask));
        El t;
        fr_mul(w.data(), heads.at(L.heads_off + pc_elem(seg + 1, l, rho)).data(), t.data());
        El& loc = heads.at(L.data_off + pc_elem(j, l, rho));
        fr_add(t.data(), loc.data(), loc.data());
    }
}
// k_pc_fix0
static void model_fix0(const ProveCosetsPlan& p, uint32_t k, Buf& q, Buf& heads, Buf& rem, bool keep) {
    const ProveLevel& L = p.level[0];
    const uint32_t l = (uint32_t)p.l, mask = (uint32_t)(p.n - 1);
    for (uint32_t x = 0; x < (keep ? L.len : 1u) * l; ++x) {
        const uint32_t rho = x & (l - 1), t = x >> p.log_l;
        if (t == 0) {
            const El w = fr_pow_w(p.log_n, pc_twist_exp(k, rho, mask));
            fr_mul(heads.at(L.heads_off + pc_elem(0, l, rho)).data(), w.data(), rem.at(rho).data());
            if (keep) q.at(pc_elem(L.len - 1, l, rho)) = {0, 0, 0, 0};
            continue;
        }
        const uint32_t seg = t >> p.log_S;
        if (seg + 1 >= L.nseg) continue;
        const El w = fr_pow_w(p.log_n, pc_pow_exp(k, L.shift, ((seg + 1) << p.log_S) - t, mask));
        El s;
        fr_mul(w.data(), heads.at(L.heads_off + pc_elem(seg + 1, l, rho)).data(), s.data());
        El& loc = q.at(pc_quot_elem(t, l, rho));
        fr_add(s.data(), loc.data(), loc.data());
    }
}

static void check_model(size_t d, size_t n, size_t l, uint32_t S, uint32_t k, bool keep) {
    snprintf(case_name, sizeof case_name, "model d=%zu n=%zu l=%zu S=%u k=%u keep=%d", d, n, l, S, k, (int)keep);
    ProveCosetsPlan p = prove_cosets_plan(d, n, l, 1, true, keep, 0);
    prove_cosets_set_levels(p, std::min<uint32_t>(S, (uint32_t)p.D));
    CHECK(p.level[p.n_levels - 1].nseg == 1);                                       // the grid stays inside PROVE_MAX_LEVELS
    // a polynomial from a fixed generator, the top quarter zero for one k
    std::vector<El> f(d);
    uint64_t s = 0x9E3779B97F4A7C15ull * (d + 3 * l + 7 * k + S);
    for (size_t i = 0; i < d; ++i) {
        El raw;
        for (auto& w : raw) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; w = s; }
        raw[3] &= 0x0FFFFFFFFFFFFFFFull;                                            // < 2^252 < r: a canonical wire word
        f[i] = (k == 1 && i >= d - d / 4) ? El{0, 0, 0, 0} : raw;
    }
    Buf q(keep ? d : 0, "quotient row"), heads(p.heads_elems, "heads"), rem(l, "remainder");
    max_products = 0;
    for (int i = 0; i < p.n_levels; ++i) model_local(p, i, k, f, q, heads, keep);
    for (int i = p.n_levels - 2; i >= 1; --i) model_fix(p, i, k, heads);
    model_fix0(p, k, q, heads, rem, keep);
    CHECK(max_products <= p.S);
    // the sequential recurrence: g = f_(rho + t l) + c g, t = D - 1 .. 0
    const uint32_t mask = (uint32_t)(n - 1);
    const El c = fr_pow_w(p.log_n, pc_mult_exp(k, p.log_l, mask));
    std::vector<El> want_q(d, El{0, 0, 0, 0}), want_r(l);
    for (size_t rho = 0; rho < l; ++rho) {
        El g = {0, 0, 0, 0};
        for (size_t t = p.D; t-- > 0;) {
            El u;
            fr_mul(c.data(), g.data(), u.data());
            fr_add(u.data(), f[rho + t * l].data(), g.data());
            if (t > 0) want_q[rho + (t - 1) * l] = g; else want_r[rho] = g;
        }
    }
    bool same = true;
    if (keep) for (size_t i = 0; i < d; ++i) same &= q.v[i] == want_q[i];
    CHECK(same);
    for (size_t rho = 0; rho < l; ++rho) {
        El tw = fr_pow_w(p.log_n, (uint32_t)(((uint64_t)k * rho) & mask)), y;
        fr_mul(want_r[rho].data(), tw.data(), y.data());
        CHECK(rem.v[rho] == y);
    }
    // and the division itself: f_i = q_(i - l) - c q_i + r_i
    bool divides = true;
    for (size_t i = 0; i < d; ++i) {
        El cq, v = i >= l ? want_q[i - l] : El{0, 0, 0, 0};
        fr_mul(c.data(), want_q[i].data(), cq.data());
        fr_sub(v.data(), cq.data(), v.data());
        if (i < l) fr_add(v.data(), want_r[i].data(), v.data());
        divides &= v == f[i];
    }
    CHECK(divides);
}

// ---- the pinned table --------------------------------------------------------------------------------------------------------------------
static void print_plan(size_t d, size_t n, size_t l, size_t items, bool values, bool quotients, size_t budget) {
    const ProveCosetsPlan p = prove_cosets_plan(d, n, l, items, values, quotients, budget);
    printf("d=%zu n=%zu l=%zu items=%zu values=%d quotients=%d budget=%zu -> S=%u levels=", d, n, l, items, (int)values, (int)quotients, budget, p.S);
    for (int i = 0; i < p.n_levels; ++i) printf("%s%u/%u", i ? "," : "", p.level[i].len, p.level[i].nseg);
    printf(" heads=%zu item_bytes=%zu group=%zu groups=%zu group_bytes=%zu launches=%u single=%d\n", p.heads_elems, p.item_bytes, p.group, p.n_groups, p.group_bytes,
           p.launches, (int)p.msm_single);
}

int main() {
    check_order();
    for (size_t d : {(size_t)2, (size_t)64, (size_t)256, (size_t)2048, (size_t)1 << 14, (size_t)1 << 16, (size_t)1 << 20, (size_t)1 << 24})
        for (size_t r : {(size_t)1, (size_t)2, (size_t)8})
            for (size_t l : {(size_t)1, (size_t)4, (size_t)16, (size_t)64, (size_t)2048, d / 2}) {
                if (l == 0 || l > d / 2 || d * r > ENCODE_MAX_N) continue;
                for (size_t items : {(size_t)0, (size_t)1, (size_t)2, (size_t)40, (size_t)100000})
                    for (int vq = 1; vq < 4; ++vq) check_plan(d, d * r, l, items, (vq & 1) != 0, (vq & 2) != 0);
            }
    for (size_t d : {(size_t)2, (size_t)4, (size_t)32, (size_t)64, (size_t)256, (size_t)1024})
        for (size_t l : {(size_t)1, (size_t)2, (size_t)8, d / 2})
            for (uint32_t S : {2u, 4u, 64u}) {
                if (l > d / 2) continue;
                const size_t D = d / l;
                if ((S == 2 && D > 32) || (S == 4 && D > 1024)) continue;          // more levels than PROVE_MAX_LEVELS: never planned (S = min(D, 64))
                const size_t n = 2 * d, m = n / l;
                for (uint32_t k : {0u, 1u, (uint32_t)(m / 2), (uint32_t)(m - 1), (uint32_t)(5 % m)}) check_model(d, n, l, S, k, true);
                check_model(d, d, l, S, (uint32_t)(d / l - 1), false);
            }
    check_model(4096, 8192, 1, 64, 4097, true);                                     // the planner's own S on two carry levels
    if (failures) return 1;
    for (size_t d : {(size_t)64, (size_t)2048, (size_t)1 << 14, (size_t)1 << 16})
        for (size_t l : {(size_t)1, (size_t)16, (size_t)2048}) {
            if (l > d / 2) continue;
            print_plan(d, 8 * d, l, 1, true, true, 0);
            print_plan(d, 8 * d, l, 256, true, true, 0);
            print_plan(d, 8 * d, l, 256, true, false, 0);
            print_plan(d, 8 * d, l, 100000, false, true, (size_t)64 << 20);
        }
    printf("provecosetscheck ok\n");
    return 0;
}
