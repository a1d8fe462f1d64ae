// tests/hostcheck/encodebatchcheck.cpp — TEST-ONLY driver for a plain g++ build (no GPU, no library) of the host side of
// kzg_encode_cosets_batch (csrc/host_encode.h EncodeBatchPlan, csrc/g1fft_plan.h with a batch).  It checks
//   1. encode_batch_check: the order of the header's table with the two new rows (count = 0 in check 1, the overflowing count last);
//   2. batch = 1 gives the plans of a single transform, field for field, over the grid of g1fft_plancheck.cpp (every log n <= 20 in every
//      direction) and every (log n, log nonzero) of the padded transform; a call of one blob plans as kzg_encode_cosets does;
//   3. group sizes are monotone in the budget, never 0, never above count, and the groups cover count;
//   4. the bytes a group reserves in every buffer hold the highest index every launch of the driver touches (the addressing of
//      multiproof_encode_batch restated here, the transform plans walked stage by stage);
//   5. the lanes the cost model assigns to a stage are grid x 256 of that stage, up to the rounding of the grid;
// and prints the plans of a small (shape, B) grid in the format of tests/golden/encode_batch_plans.txt.  Built and run by
// tests/test_encode_batch_plan_host.py, plain and under ASan + UBSan.  Exit status 1 and a line on stderr per violated check.
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>

#include "host_encode.h"

using namespace kzg;

static int failures = 0;
static char case_name[256] = "";
#define CHECK(c) do { if (!(c)) { ++failures; fprintf(stderr, "encodebatchcheck: %s: line %d: %s\n", case_name, __LINE__, #c); } } while (0)

static bool same_stage(const G1fftStage& a, const G1fftStage& b) {
    return a.kind == b.kind && a.K == b.K && a.log_s == b.log_s && a.last == b.last && a.grid == b.grid && a.Q == b.Q && a.wpo == b.wpo && a.scal == b.scal &&
           a.partials == b.partials && a.src == b.src && a.dst == b.dst;
}
static bool same_plan(const G1fftPlan& a, const G1fftPlan& b) {
    bool ok = a.n == b.n && a.log_n == b.log_n && a.form == b.form && a.n_stages == b.n_stages && a.sum_grid == b.sum_grid && a.n_scal_keys == b.n_scal_keys &&
              a.t3 == b.t3 && a.t3_points == b.t3_points && a.naf == b.naf && a.tab_small == b.tab_small && a.tab_c == b.tab_c && a.tab_W == b.tab_W &&
              a.bytes_a == b.bytes_a && a.bytes_b == b.bytes_b && a.bytes_c == b.bytes_c && a.result == b.result && a.batch == b.batch;
    for (int i = 0; ok && i < a.n_stages; ++i) ok = same_stage(a.stage[i], b.stage[i]);
    for (int i = 0; ok && i < a.n_scal_keys; ++i) ok = a.scal_keys[i] == b.scal_keys[i];
    return ok;
}

// ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
static void check_order() {
    snprintf(case_name, sizeof case_name, "order");
    const size_t SRS = 3000;
    // a valid call
    CHECK(encode_batch_check(false, false, 1, 64, 128, 1, SRS) == KZG_OK);
    CHECK(encode_batch_check(false, false, 1000, 2048, 1 << 24, 1024, SRS) == KZG_OK);
    // 1. pointers and count = 0 in front of everything
    CHECK(encode_batch_check(true, true, 0, 3, 0, 0, 0) == KZG_ERR_INVALID_ARG);
    CHECK(encode_batch_check(false, false, 0, 3, 0, 1, SRS) == KZG_ERR_INVALID_ARG);            // count = 0 in front of a length that is no power of two
    CHECK(encode_batch_check(false, false, 0, 64, 128, 1, SRS) == KZG_ERR_INVALID_ARG);
    // 2. the SRS in front of the lengths
    CHECK(encode_batch_check(false, true, 1, 3, 0, 1, SRS) == KZG_ERR_INVALID_ARG);
    // 3. lengths in front of the domain limit
    CHECK(encode_batch_check(false, false, 1, 0, 64, 1, SRS) == KZG_ERR_NOT_POWER_OF_TWO);
    CHECK(encode_batch_check(false, false, 1, 48, (size_t)1 << 25, 1, SRS) == KZG_ERR_NOT_POWER_OF_TWO);
    CHECK(encode_batch_check(false, false, 1, 64, 96, 1, SRS) == KZG_ERR_NOT_POWER_OF_TWO);
    // 4. the domain limit in front of the shape rules
    CHECK(encode_batch_check(false, false, 1, 1, (size_t)1 << 25, 3, SRS) == KZG_ERR_DOMAIN);
    // 5. shapes in front of the capacity
    CHECK(encode_batch_check(false, false, 1, 4096, 2048, 1, SRS) == KZG_ERR_INVALID_ARG);
    CHECK(encode_batch_check(false, false, 1, 1, 64, 1, SRS) == KZG_ERR_INVALID_ARG);
    CHECK(encode_batch_check(false, false, 1, 4096, 4096, 3, SRS) == KZG_ERR_INVALID_ARG);
    CHECK(encode_batch_check(false, false, 1, 64, 4096, 64, SRS) == KZG_ERR_INVALID_ARG);
    // 6. the capacity in front of the overflow
    CHECK(encode_batch_check(false, false, 1, 4096, 4096, 1, SRS) == KZG_ERR_SRS_CAPACITY_EXCEEDED);
    CHECK(encode_batch_check(false, false, SIZE_MAX, 4096, 4096, 1, SRS) == KZG_ERR_SRS_CAPACITY_EXCEEDED);
    // 7. a count whose outputs overflow size_t: count x n x 64 bytes
    CHECK(encode_batch_check(false, false, SIZE_MAX, 64, 128, 1, SRS) == KZG_ERR_INVALID_ARG);
    CHECK(encode_batch_check(false, false, SIZE_MAX / (128 * 64) + 1, 64, 128, 1, SRS) == KZG_ERR_INVALID_ARG);
    CHECK(encode_batch_check(false, false, SIZE_MAX / (128 * 64), 64, 128, 1, SRS) == KZG_OK);
    // every error of encode_check is the error of the batch check with count = 1
    for (size_t d : {(size_t)0, (size_t)1, (size_t)2, (size_t)48, (size_t)64, (size_t)4096})
        for (size_t n : {(size_t)0, (size_t)64, (size_t)96, (size_t)4096, (size_t)1 << 25})
            for (size_t l : {(size_t)0, (size_t)1, (size_t)3, (size_t)32, (size_t)64})
                CHECK(encode_batch_check(false, false, 1, d, n, l, SRS) == encode_check(false, false, d, n, l, SRS));
}

// ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
static void check_batch_one() {
    for (int log_n = 0; log_n <= 20; ++log_n) {
        const size_t n = (size_t)1 << log_n;
        int k0 = -1, k1 = -2;
        bool p0 = false, p1 = true;
        snprintf(case_name, sizeof case_name, "batch-one log_n=%d", log_n);
        g1fft_choose_plan(n, log_n, &k0, &p0);
        g1fft_choose_plan_batch(n, log_n, 1, &k1, &p1);
        CHECK(k0 == k1 && p0 == p1);
        for (int inverse = 0; inverse < 2; ++inverse)
            for (int scaled = 0; scaled < 2; ++scaled)
                for (int strided = 0; strided < 2; ++strided)
                    CHECK(same_plan(g1fft_plan_planes(n, inverse != 0, scaled != 0, strided != 0), g1fft_plan_planes(n, inverse != 0, scaled != 0, strided != 0, 1)));
        for (int log_nz = 0; log_nz <= log_n; ++log_nz) {
            const G1fftPaddedPlan a = g1fft_plan_planes_padded(n, (size_t)1 << log_nz), b = g1fft_plan_planes_padded(n, (size_t)1 << log_nz, 1);
            CHECK(same_plan(a.plan, b.plan) && a.nonzero == b.nonzero && a.log_nonzero == b.log_nonzero && a.log_r == b.log_r);
        }
    }
    // one blob: the plan of kzg_encode_cosets, whatever the budget
    for (size_t d : {(size_t)2, (size_t)256, (size_t)4096, (size_t)65536})
        for (size_t r : {(size_t)1, (size_t)2, (size_t)8})
            for (size_t l : {(size_t)1, (size_t)16, (size_t)128})
                for (size_t budget : {(size_t)0, (size_t)1}) {
                    if (l > d / 2) continue;
                    snprintf(case_name, sizeof case_name, "one-blob d=%zu r=%zu l=%zu", d, r, l);
                    const EncodeBatchPlan bp = encode_batch_plan(d, d * r, l, 1, true, true, budget);
                    const EncodePlan one = encode_plan(d, d * r, l, true, true);
                    CHECK(bp.group == 1 && bp.n_groups == 1);
                    CHECK(same_plan(bp.fft.plan, one.fft.plan) && same_plan(bp.ifft, g1fft_plan_planes(one.M, true, true, false)));
                    for (int i = 0; i < 6; ++i) CHECK(bp.bytes[i] == one.bytes[i]);
                }
}

// ---- 4: the highest byte + 1 the launches of a group of g blobs touch in mp[i], the addressing of multiproof_encode_batch ----------------
static size_t planes_words(size_t points) { return points * 4 * ENCODE_LIMBS; }            // a plane set of stride `points` holds 36 planes
static void walk_transform(const G1fftPlan& p, int out_set, int tmp_set, size_t need_points[3]) {
    for (int i = 0; i < p.n_stages; ++i) {
        const int buf = p.stage[i].dst;                                                       // the buffers are named so that the plan ends in `out`
        const int set = buf == p.result ? out_set : tmp_set;
        need_points[set] = std::max<size_t>(need_points[set], p.n);                           // every stage writes n points of stride n
        CHECK(p.stage[i].grid * (size_t)p.batch <= (size_t)UINT_MAX && p.batch <= 65535);
    }
}
static void check_group_bytes(const EncodeBatchPlan& bp, size_t g) {
    const EncodePlan& p = bp.one;
    size_t top[6] = {0, 0, 0, 0, 0, 0};
    top[0] = g * bp.f_stride * ENCODE_FR_BYTES;                                               // g rows of f_stride coefficients
    CHECK(bp.f_stride >= p.d && (!p.values || bp.f_stride == p.n));
    if (bp.f_stride != p.d) top[1] = std::max(top[1], g * p.d * ENCODE_FR_BYTES);             // the compact upload
    if (p.proofs) top[1] = std::max(top[1], g * p.l * p.M * ENCODE_FR_BYTES);                 // g l rows of 2m'
    if (p.values) top[1] = std::max(top[1], g * p.n * ENCODE_FR_BYTES);                       // g rows of coset-major values
    if (p.proofs) {
        size_t need[3] = {0, 0, 0};
        const int h = p.lincomb.W > 1 ? 1 : 0, x = 1 - h;
        need[0] = p.l == 1 ? p.M : p.M * p.lincomb.W;                                         // the linear combination's slots (H itself when W = 1)
        need[h] = std::max(need[h], p.M);                                                     // H
        walk_transform(bp.ifft, x, 2, need);                                                  // H -> X, scratch in set 2
        CHECK(bp.ifft.n == p.M && bp.fft.plan.n == p.m && bp.fft.nonzero == p.mp);
        // the slice of X the forward transform reads in place: offset m' - 1, stride 2m', m' points of 36 planes
        CHECK((p.mp - 1) + 35 * p.M + (p.mp - 1) < planes_words(need[x]));
        walk_transform(bp.fft.plan, h, 2, need);                                              // slice of X -> Y = the set H was in
        for (int i = 0; i < 3; ++i) {
            CHECK(need[i] <= bp.set_points[i]);                                               // a blob stays inside its own plane set
            top[2 + i] = ((g - 1) * planes_words(bp.set_points[i]) + planes_words(need[i])) * 4;
        }
        top[5] = g * p.m * (ENCODE_AFFINE_BYTES + ENCODE_LIMBS * 4 + 1);
    }
    size_t sum = 0;
    for (int i = 0; i < 6; ++i) {
        CHECK(top[i] <= bp.bytes[i]);
        CHECK(bp.bytes[i] == bp.blob_bytes[i] * g);
        sum += bp.bytes[i];
    }
    // the Fr NTT workspaces: rows x n x 32 bytes per buffer a multi-pass transform uses
    size_t ntt[2] = {0, 0};
    auto rows_of = [&](int log_n, size_t rows) {
        if (log_n < 1) return;
        const int passes = (log_n + NTT_KMAX - 1) / NTT_KMAX;
        if (passes > 1) ntt[0] = std::max(ntt[0], (rows << log_n) * 32);
        if (passes > 2) ntt[1] = std::max(ntt[1], (rows << log_n) * 32);
    };
    if (p.proofs) rows_of(g1fft_log2(p.M), p.l * g);
    if (p.values) rows_of(p.log_n, g);
    rows_of(p.log_d, g);
    CHECK(ntt[0] <= bp.ntt_bytes[0] && ntt[1] <= bp.ntt_bytes[1]);
    CHECK(bp.group_bytes == sum + bp.ntt_bytes[0] + bp.ntt_bytes[1]);
}

// ---- 5: model lanes of a stage = grid x 256, up to the rounding of the grid ------------------------------------------------------------------
static void check_model_lanes(const G1fftPlan& p) {
    for (int i = 0; i < p.n_stages; ++i) {
        const G1fftStage& s = p.stage[i];
        size_t lanes = 0;
        switch (s.kind) {
        case G1S_DIRECT: lanes = (size_t)p.n << s.K; break;
        case G1S_DIRECT_PAIRS: lanes = 2 * ((size_t)p.n << s.K); break;
        case G1S_RADIX2: lanes = p.n / 2; break;
        case G1S_RADIX2_PAIRS: lanes = p.n; break;
        default: lanes = p.n; break;                                                          // copies: one lane per point
        }
        CHECK(s.grid * 256 >= lanes && s.grid * 256 < lanes + 256);                           // per transform; the batch is grid.y
        CHECK(s.grid * 256 * p.batch >= lanes * p.batch && s.grid * 256 * p.batch < (lanes + 256) * p.batch);
    }
}

// ---- 3, 4, 5 over a grid of shapes, counts and budgets ---------------------------------------------------------------------------------
static void check_groups() {
    const size_t counts[] = {1, 2, 3, 7, 8, 64, 1000, 100000};
    for (size_t d : {(size_t)2, (size_t)64, (size_t)256, (size_t)1024, (size_t)4096, (size_t)16384, (size_t)65536})
        for (size_t r : {(size_t)1, (size_t)2, (size_t)8})
            for (size_t l : {(size_t)1, (size_t)16, (size_t)128, (size_t)512})
                for (int outs = 1; outs <= 3; ++outs) {
                    if (l > d / 2) continue;
                    const bool values = (outs & 1) != 0, proofs = (outs & 2) != 0;
                    const size_t one = encode_batch_plan(d, d * r, l, 2, values, proofs, 1).group_bytes;   // budget 1: a group of one blob
                    for (size_t count : counts) {
                        size_t prev = 0;
                        size_t budgets[] = {1, one - 1, one, 2 * one - 1, 2 * one, 3 * one + one / 2, 7 * one, 64 * one, (size_t)1 << 30, 0 /* the default */, (size_t)1 << 36};
                        std::sort(budgets, budgets + sizeof budgets / sizeof *budgets, [](size_t a, size_t b) { return (a ? a : ENCODE_GROUP_BYTES_DEFAULT) < (b ? b : ENCODE_GROUP_BYTES_DEFAULT); });
                        for (size_t budget : budgets) {
                            snprintf(case_name, sizeof case_name, "d=%zu r=%zu l=%zu count=%zu values=%d proofs=%d budget=%zu", d, r, l, count, (int)values, (int)proofs, budget);
                            const EncodeBatchPlan bp = encode_batch_plan(d, d * r, l, count, values, proofs, budget);
                            CHECK(bp.group >= 1 && bp.group <= count && bp.group <= ENCODE_GROUP_MAX);
                            CHECK(bp.n_groups >= 1 && (bp.n_groups - 1) * bp.group < count && bp.n_groups * bp.group >= count);
                            CHECK(bp.group >= prev);                                           // monotone in the budget
                            prev = bp.group;
                            CHECK(bp.group == 1 || bp.group_bytes <= bp.budget);               // within the budget unless one blob alone exceeds it
                            CHECK(bp.group == 1 || bp.batched);
                            if (!bp.batched) CHECK(proofs && bp.min_stage_lanes >= ENCODE_STAGE_LANE_CAP && bp.group == 1);
                            if (bp.batched && proofs) CHECK(bp.min_stage_lanes < ENCODE_STAGE_LANE_CAP);
                            if (budget == 3 * one + one / 2 && bp.batched) CHECK(bp.group == std::min<size_t>(count, 3));
                            check_group_bytes(bp, bp.group);
                            if (proofs) {
                                CHECK(bp.ifft.batch == bp.group && bp.fft.plan.batch == bp.group);
                                check_model_lanes(bp.ifft);
                                check_model_lanes(bp.fft.plan);
                            }
                            // the last, smaller group of a call is sized and planned like a call of that many blobs
                            const size_t tail = count - (bp.n_groups - 1) * bp.group;
                            if (tail != bp.group) {
                                EncodeBatchPlan t = bp;
                                encode_batch_size_group(t, tail);
                                check_group_bytes(t, tail);
                                for (int i = 0; i < 6; ++i) CHECK(t.bytes[i] <= bp.bytes[i]);  // it fits what the call reserved
                            }
                        }
                    }
                }
}

// ---- the pinned plans ----------------------------------------------------------------------------------------------------------------------
static const char* const KIND[G1S_KINDS] = {"load", "load_bitrev", "gather", "gather_bitrev", "bits", "first_tables", "direct", "direct_pairs", "mul_quads",
                                            "radix2", "radix2_pairs", "pad", "spread"};
static const char* const FORM[G1FFT_FORMS] = {"copy", "bits", "bits+quads", "tables+direct", "direct", "radix2"};
static void print_transform(const char* name, const G1fftPlan& p) {
    printf("  %s n=%u form=%s batch=%u result=%d:", name, p.n, FORM[p.form], p.batch, p.result);
    for (int i = 0; i < p.n_stages;) {
        const G1fftStage& s = p.stage[i];
        int run = 1;                                                                          // consecutive radix-2 stages differ in their number only
        while ((s.kind == G1S_RADIX2 || s.kind == G1S_RADIX2_PAIRS) && i + run < p.n_stages && p.stage[i + run].kind == s.kind && p.stage[i + run].grid == s.grid &&
               p.stage[i + run].log_s == s.log_s + run) ++run;
        if (run > 1) printf(" %s[s=%d..%d grid=%zu]", KIND[s.kind], s.log_s, s.log_s + run - 1, s.grid);
        else printf(" %s[K=%d log_s=%d grid=%zu]", KIND[s.kind], s.K, s.log_s, s.grid);
        i += run;
    }
    printf("\n");
}
static void print_plans() {
    struct Case { size_t d, n, l, count, budget; bool values, proofs; };
    const Case cases[] = {
        {2, 4, 1, 3, 0, true, true},           {64, 128, 1, 5, 0, true, true},         {256, 2048, 16, 8, 0, true, true},    {256, 2048, 1, 4, 0, true, true},
        {1024, 2048, 512, 3, 0, true, true},   {512, 512, 128, 3, 0, true, true},      {256, 2048, 16, 7, 926912, true, true}, {256, 2048, 16, 7, 1, true, true},
        {1024, 2048, 1, 2, 0, true, true},     {1024, 2048, 1, 8, 0, true, true},      {1024, 2048, 1, 16, 0, true, true},   {1024, 8192, 1, 16, 0, true, true},
        {4096, 32768, 16, 1, 0, true, true},   {4096, 32768, 16, 4, 0, true, true},    {4096, 32768, 16, 8, 0, true, true},  {4096, 32768, 16, 16, 0, true, true},
        {4096, 32768, 16, 64, 0, true, true},  {4096, 4096, 16, 64, 0, true, true},    {4096, 32768, 1, 16, 0, true, true},  {16384, 131072, 16, 64, 0, true, true},
        {16384, 131072, 1, 64, 0, true, true}, {65536, 524288, 16, 64, 0, true, true}, {65536, 524288, 1, 16, 0, true, true}, {65536, 65536, 1, 4, 0, true, true},
        {4096, 32768, 16, 16, 0, true, false}, {4096, 32768, 16, 16, 0, false, true},  {65536, 524288, 1, 16, 0, true, false},
    };
    for (const Case& c : cases) {
        const EncodeBatchPlan bp = encode_batch_plan(c.d, c.n, c.l, c.count, c.values, c.proofs, c.budget);
        printf("d=%zu n=%zu l=%zu count=%zu budget=%zu values=%d proofs=%d -> batched=%d min_stage_lanes=%zu group=%zu groups=%zu group_bytes=%zu f_stride=%zu\n", c.d, c.n, c.l,
               c.count, c.budget, (int)c.values, (int)c.proofs, (int)bp.batched, bp.min_stage_lanes, bp.group, bp.n_groups, bp.group_bytes, bp.f_stride);
        printf("  bytes=%zu,%zu,%zu,%zu,%zu,%zu ntt=%zu,%zu set_points=%zu,%zu,%zu lincomb=2^%d x %u x %u\n", bp.bytes[0], bp.bytes[1], bp.bytes[2], bp.bytes[3], bp.bytes[4],
               bp.bytes[5], bp.ntt_bytes[0], bp.ntt_bytes[1], bp.set_points[0], bp.set_points[1], bp.set_points[2], bp.one.lincomb.log_g, bp.one.lincomb.W, bp.one.lincomb.tpl);
        if (c.proofs) {
            print_transform("inverse", bp.ifft);
            print_transform("forward", bp.fft.plan);
        }
    }
}

int main() {
    check_order();
    check_batch_one();
    check_groups();
    print_plans();
    if (failures) { fprintf(stderr, "encodebatchcheck: %d checks failed\n", failures); return 1; }
    printf("encodebatchcheck ok\n");
    return 0;
}
