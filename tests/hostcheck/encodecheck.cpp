// encodecheck.cpp -- csrc/host_encode.h as a plain host program (g++ -fsanitize=address,undefined, no GPU, no library): every error of
// kzg_encode_cosets' documented table in its order, the sizes and workspace bytes of fixed shapes, and what the driver and the kernels
// rely on in the plan of the zero-padded transform.  Prints "encodecheck ok"; a failed check prints its line and exits 1.
#include <cstdio>
#include <cstdlib>

#include "host_encode.h"

using namespace kzg;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "encodecheck: line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)

static bool same_stage(const G1fftStage& a, const G1fftStage& b) {
    return a.kind == b.kind && a.K == b.K && a.log_s == b.log_s && a.last == b.last && a.grid == b.grid && a.Q == b.Q && a.wpo == b.wpo && a.scal == b.scal &&
           a.partials == b.partials && a.src == b.src && a.dst == b.dst;
}
static bool same_plan(const G1fftPlan& a, const G1fftPlan& b) {
    bool ok = a.n == b.n && a.log_n == b.log_n && a.form == b.form && a.n_stages == b.n_stages && a.sum_grid == b.sum_grid && a.n_scal_keys == b.n_scal_keys &&
              a.t3 == b.t3 && a.t3_points == b.t3_points && a.naf == b.naf && a.tab_small == b.tab_small && a.tab_c == b.tab_c && a.tab_W == b.tab_W &&
              a.bytes_a == b.bytes_a && a.bytes_b == b.bytes_b && a.bytes_c == b.bytes_c && a.result == b.result;
    for (int i = 0; ok && i < a.n_stages; ++i) ok = same_stage(a.stage[i], b.stage[i]);
    for (int i = 0; ok && i < a.n_scal_keys; ++i) ok = a.scal_keys[i] == b.scal_keys[i];
    return ok;
}
static int lanes_per_point(G1fftStageKind k) { return k == G1S_RADIX2_PAIRS || k == G1S_DIRECT_PAIRS ? 2 : 1; }

// what g1_fft_planes_padded and its kernels rely on, for an m-point transform with m / r points that are not the identity
static void check_padded(int log_m, int log_r) {
    const size_t m = (size_t)1 << log_m, nz = m >> log_r;
    const G1fftPaddedPlan pp = g1fft_plan_planes_padded(m, nz);
    const G1fftPlan& p = pp.plan;
    const G1fftPlan full = g1fft_plan_planes(m, false, false, true);
    CHECK(pp.nonzero == nz && pp.log_r == log_r && ((size_t)1 << pp.log_nonzero) == nz);           // the spread factor is r
    CHECK(p.n == m && p.log_n == log_m && p.form == full.form && p.result == full.result);
    CHECK(p.n_scal_keys == 1 && p.scal_keys[0] == G1SCAL_FORWARD);
    if (log_r == 0) { CHECK(same_plan(p, full)); return; }                                         // r = 1: the plan of g1_fft_planes
    int kmax = 0; bool pairs = false;
    g1fft_choose_plan(m, log_m, &kmax, &pairs);
    CHECK(p.stage[0].src == G1BUF_INPUT && p.stage[0].dst == 0 && p.stage[0].K == 0 && p.stage[0].scal < 0 && p.stage[0].grid * 256 >= m && (p.stage[0].grid - 1) * 256 < m);
    if (p.form == G1FFT_RADIX2) {
        CHECK(kmax == 0 && p.stage[0].kind == G1S_SPREAD_BITREV && p.stage[0].log_s == log_r);
        CHECK(p.n_stages == 1 + log_m - log_r && p.result == 0);                                   // exactly log2 m - log2 r butterfly stages ...
        for (int i = 1; i < p.n_stages; ++i) {
            const G1fftStage& s = p.stage[i];
            CHECK(s.kind == (pairs ? G1S_RADIX2_PAIRS : G1S_RADIX2) && s.K == 1 && s.log_s == log_r + i);      // ... numbered from log2 r + 1
            CHECK(s.src == 0 && s.dst == 0 && !s.last && s.scal == G1SCAL_FORWARD && !s.partials);
            const size_t lanes = m / 2 * lanes_per_point(s.kind);                                  // m / 2 butterflies times the lanes of a point
            CHECK(s.grid * 256 >= lanes && (s.grid - 1) * 256 < lanes);
            CHECK(same_stage(s, full.stage[log_r + i]));                                           // the stage of the full transform, unchanged
        }
        CHECK(p.stage[p.n_stages - 1].log_s == log_m);
    } else {
        CHECK(kmax >= 2 && p.form == G1FFT_DIRECT && p.stage[0].kind == G1S_GATHER_PAD && p.n_stages == full.n_stages);
        for (int i = 1; i < p.n_stages; ++i) CHECK(same_stage(p.stage[i], full.stage[i]));        // pruning inside the direct stages is not done
    }
}

static const size_t PT = G1FFT_POINT_BYTES, AFF = 64 + 1 + 9 * 4;

int main() {
    const size_t BIG = (size_t)1 << 25;
    // ---- the error table, each case wrong in its own check AND in a later one: the earlier wins
    CHECK(encode_check(true, false, 0, 0, 0, 0) == KZG_ERR_INVALID_ARG);                // 1. a null pointer / no output / proofs without flags, in front of a bad n
    CHECK(encode_check(false, true, 0, 0, 0, 0) == KZG_ERR_INVALID_ARG);                // 2. a foreign or Lagrange SRS, in front of a bad n
    CHECK(encode_check(false, false, 0, 8, 1, 0) == KZG_ERR_NOT_POWER_OF_TWO);          // 3. poly_len = 0
    CHECK(encode_check(false, false, 3, BIG, 1, 0) == KZG_ERR_NOT_POWER_OF_TWO);        //    poly_len not a power of two, in front of the domain limit
    CHECK(encode_check(false, false, 4, 0, 1, 0) == KZG_ERR_NOT_POWER_OF_TWO);          //    n = 0
    CHECK(encode_check(false, false, 4, 24, 1, 0) == KZG_ERR_NOT_POWER_OF_TWO);         //    n not a power of two
    CHECK(encode_check(false, false, 1, BIG, 3, 0) == KZG_ERR_DOMAIN);                  // 4. n > 2^24, in front of poly_len = 1 and a bad chunk length
    CHECK(encode_check(false, false, 16, 8, 1, 0) == KZG_ERR_INVALID_ARG);              // 5. poly_len > n, in front of the SRS capacity
    CHECK(encode_check(false, false, 1, 8, 1, 0) == KZG_ERR_INVALID_ARG);               //    poly_len = 1
    CHECK(encode_check(false, false, 8, 8, 0, 0) == KZG_ERR_INVALID_ARG);               //    chunk_len = 0
    CHECK(encode_check(false, false, 8, 8, 3, 0) == KZG_ERR_INVALID_ARG);               //    chunk_len not a power of two
    CHECK(encode_check(false, false, 8, 64, 8, 0) == KZG_ERR_INVALID_ARG);              //    chunk_len > poly_len / 2 (n / 2 would allow it)
    CHECK(encode_check(false, false, 8, 64, 4, 7) == KZG_ERR_SRS_CAPACITY_EXCEEDED);    // 6. poly_len > the SRS
    CHECK(encode_check(false, false, 8, 64, 4, 8) == KZG_OK);                           //    an SRS of d points, n beyond it
    CHECK(encode_check(false, false, 2, (size_t)1 << 24, 1, 2) == KZG_OK);              //    the largest domain

    // ---- sizes and workspace bytes
    {
        const EncodePlan p = encode_plan(2, 2, 1, true, true);
        CHECK(p.m == 2 && p.mp == 2 && p.r == 1 && p.M == 4 && p.log_m == 1 && p.log_r == 0 && p.lincomb.W == 1 && p.lincomb.log_g == 0 && p.lincomb.tpl == 1);
        CHECK(p.bytes[0] == 2 * 32 && p.bytes[1] == 4 * 32 && p.bytes[2] == 4 * PT && p.bytes[3] == 4 * PT && p.bytes[4] == 4 * PT && p.bytes[5] == 2 * AFF);
        CHECK(same_plan(p.fft.plan, g1fft_plan_planes(2, false, false, true)));
    }
    {
        const size_t n = (size_t)1 << 15;
        const EncodePlan p = encode_plan(2, n, 1, true, true);
        CHECK(p.m == n && p.mp == 2 && p.r == n / 2 && p.M == 4 && p.log_r == 14 && p.log_m == 15);
        CHECK(p.bytes[0] == n * 32 && p.bytes[1] == n * 32 && p.bytes[2] == n * PT && p.bytes[3] == n * PT && p.bytes[4] == n * PT && p.bytes[5] == n * AFF);
        CHECK(p.fft.plan.form == G1FFT_RADIX2 && p.fft.plan.n_stages == 2 && p.fft.plan.stage[1].kind == G1S_RADIX2_PAIRS && p.fft.plan.stage[1].log_s == 15);
    }
    {
        const size_t d = (size_t)1 << 12, n = (size_t)1 << 15;
        const EncodePlan p = encode_plan(d, n, 1, true, true);
        CHECK(p.m == n && p.mp == d && p.r == 8 && p.M == 2 * d && p.log_r == 3);
        CHECK(p.bytes[0] == n * 32 && p.bytes[1] == n * 32 && p.bytes[2] == n * PT && p.bytes[3] == n * PT && p.bytes[4] == n * PT && p.bytes[5] == n * AFF);
        CHECK(p.fft.plan.form == G1FFT_RADIX2 && p.fft.plan.n_stages == 13 && p.fft.plan.stage[1].kind == G1S_RADIX2_PAIRS && p.fft.plan.stage[1].log_s == 4);
        const EncodePlan q = encode_plan(d, n, 1, false, true);                                     // proofs only: no n x 32 B of values
        CHECK(q.bytes[0] == d * 32 && q.bytes[1] == 2 * d * 32 && q.bytes[2] == n * PT && q.bytes[5] == n * AFF);
        const EncodePlan v = encode_plan(d, n, 1, true, false);                                     // values only: no plane set
        CHECK(v.bytes[0] == n * 32 && v.bytes[1] == n * 32 && v.bytes[2] == 0 && v.bytes[3] == 0 && v.bytes[4] == 0 && v.bytes[5] == 0);
    }
    {
        const size_t d = (size_t)1 << 14, n = (size_t)1 << 17;
        const EncodePlan p = encode_plan(d, n, 1, true, true);
        CHECK(p.m == n && p.mp == d && p.r == 8 && p.M == 2 * d);
        CHECK(p.bytes[0] == n * 32 && p.bytes[1] == n * 32 && p.bytes[2] == n * PT && p.bytes[3] == n * PT && p.bytes[4] == n * PT && p.bytes[5] == n * AFF);
        CHECK(p.fft.plan.form == G1FFT_RADIX2 && p.fft.plan.n_stages == 15 && p.fft.plan.stage[1].kind == G1S_RADIX2 && p.fft.plan.stage[1].grid == n / 2 / 256);
    }
    {
        const EncodePlan p = encode_plan(2048, 4096, 16, true, true);
        CHECK(p.m == 256 && p.mp == 128 && p.r == 2 && p.M == 256 && p.log_l == 4 && p.log_m == 8 && p.lincomb.log_g == 4 && p.lincomb.W == 1 && p.lincomb.tpl == 1);
        CHECK(p.bytes[0] == 4096 * 32 && p.bytes[1] == 4096 * 32 && p.bytes[2] == 256 * PT && p.bytes[3] == 256 * PT && p.bytes[4] == 256 * PT && p.bytes[5] == 256 * AFF);
        CHECK(p.fft.plan.form == G1FFT_DIRECT && p.fft.plan.stage[0].kind == G1S_GATHER_PAD && p.fft.nonzero == 128);
    }
    {   // l > 64: the partial sums of the linear combination are the largest plane set
        const EncodePlan p = encode_plan(1024, 2048, 512, true, true);
        CHECK(p.m == 4 && p.mp == 2 && p.M == 4 && p.lincomb.log_g == 6 && p.lincomb.W == 8 && p.lincomb.tpl == 1 && p.bytes[2] == 32 * PT && p.bytes[3] == 4 * PT);
        const Fk20Shape s = fk20_shape(4096);
        CHECK(s.log_g == 6 && s.W == 32 && s.tpl == 2);
    }

    // ---- the plan of the padded transform: every m up to 2^24 with every r that leaves two points or more (m' = d / l >= 2)
    for (int log_m = 1; log_m <= 24; ++log_m)
        for (int log_r = 0; log_r < log_m; ++log_r) check_padded(log_m, log_r);
    printf("encodecheck ok\n");
    return 0;
}
