// tests/hostcheck/g1fft_plancheck.cpp — TEST-ONLY driver for a plain g++ build (no GPU, no library) of csrc/g1fft_plan.h: prints the plan of
// every case of the fixed grid (g1fft_grid.h) in the format of tests/golden/g1fft_plans.txt and checks, on every plan, what the kernels of
// g1fft.hip rely on whatever the policy decides.  Built and run by tests/test_g1fft_plan_host.py and, under ASan + UBSan, by
// tests/test_sanitizers_host.py.  Exit status 1 and a line on stderr per violated invariant.
#include <climits>
#include <cstdio>
#include <cstring>

#include "g1fft_plan.h"
#include "g1fft_grid.h"

using namespace kzg;

static int failures = 0;
static char case_name[96];
#define INVARIANT(c) do { if (!(c)) { ++failures; fprintf(stderr, "g1fft_plancheck: %s: %s\n", case_name, #c); } } while (0)

static const char* const KERNEL[G1S_KINDS] = {"k_g1fft_load", "k_g1fft_load", "k_g1fft_gather_planes", "k_g1fft_gather_planes", "k_g1fft_bits", "k_g1fft_first_tables",
                                              "k_g1fft_direct", "k_g1fft_direct_pairs", "k_g1fft_mul_quads", "k_g1fft_stage", "k_g1fft_stage_pairs"};
static const char* const FORM[G1FFT_FORMS] = {"copy", "bits", "bits+quads", "tables+direct", "direct", "radix2"};
static const int LANES_PER_POINT[G1S_KINDS] = {1, 1, 1, 1, 0, 0, 1, 2, 4, 1, 2};

// names[0 .. 2]: the input, plane buffer 0, plane buffer 1
static void print_plan(const G1fftPlan& p, const char* const names[3]) {
    bool has[G1S_KINDS] = {};
    for (int i = 0; i < p.n_stages; ++i) has[p.stage[i].kind] = true;
    const char* form = g1fft_form_of(has[G1S_BITS], has[G1S_MUL_QUADS], has[G1S_FIRST_TABLES], has[G1S_DIRECT] || has[G1S_DIRECT_PAIRS], has[G1S_RADIX2] || has[G1S_RADIX2_PAIRS]);
    INVARIANT(strcmp(form, FORM[p.form]) == 0);
    g1fft_print_plan(form, p.n_stages, p.bytes_a, p.bytes_b, p.bytes_c, names[1 + p.result], p.scal_keys, p.n_scal_keys, p.naf, p.t3_points,
                     p.tab_W ? (p.tab_small ? "small" : "points") : "none", p.tab_c, p.tab_W);
    for (int i = 0; i < p.n_stages; ++i) {
        const G1fftStage& s = p.stage[i];
        const bool bitrev = s.kind == G1S_LOAD_BITREV || s.kind == G1S_GATHER_BITREV;
        g1fft_print_stage(KERNEL[s.kind], s.grid, s.K, s.log_s, bitrev ? p.log_n : 0, (int)s.last, s.scal, s.Q, s.wpo, s.partials, s.partials ? p.sum_grid : 0,
                          names[1 + s.src], names[1 + s.dst]);
    }
    g1fft_end_case();
}

static void check_invariants(const G1fftPlan& p, bool planes) {
    const size_t n = p.n;
    INVARIANT(n == (size_t)1 << p.log_n && p.n_stages >= 1 && p.n_stages <= G1FFT_MAX_STAGES);
    int bits_sum = 0, bits_stages = 0;
    size_t max_partial_points = 0;
    int holds = G1BUF_INPUT;                                       // the buffer that holds the data so far
    for (int i = 0; i < p.n_stages; ++i) {
        const G1fftStage& s = p.stage[i];
        const size_t R = (size_t)1 << s.K;
        bits_sum += s.K;
        INVARIANT(s.grid >= 1 && s.grid <= UINT_MAX);                                          // every (unsigned) grid cast fits
        INVARIANT(s.src == holds && (s.dst == 0 || s.dst == 1));                               // each stage reads what the one before wrote
        INVARIANT(s.src == G1BUF_INPUT || s.scal >= 0);
        holds = s.dst;
        if (s.partials) {
            INVARIANT(s.partials >= 1 && s.partials <= 32);                                    // k_g1fft_sum_partials adds at most 32 partials per output
            INVARIANT(p.sum_grid <= UINT_MAX && p.sum_grid * 256 >= n * 64);                   // one wave per output
            max_partial_points = std::max(max_partial_points, n * s.partials);
        }
        INVARIANT(s.scal < G1SCAL_KEYS);
        if (s.scal >= 0) {                                                                     // the table a stage reads is one the plan fetches
            bool fetched = false;
            for (int k = 0; k < p.n_scal_keys; ++k) fetched |= p.scal_keys[k] == s.scal;
            INVARIANT(fetched);
        }
        switch (s.kind) {
        case G1S_LOAD: case G1S_LOAD_BITREV: case G1S_GATHER: case G1S_GATHER_BITREV:
            INVARIANT(i == 0 && s.K == 0 && s.scal < 0 && !s.partials && s.grid * 256 >= n);
            INVARIANT(planes == (s.kind == G1S_GATHER || s.kind == G1S_GATHER_BITREV));
            break;
        case G1S_BITS:
            ++bits_stages;
            INVARIANT(i == 0 && !planes && s.Q >= 1 && (R * s.Q) % 32 == 0 && s.wpo == R * s.Q / 32);   // slot < R Q: whole waves of 32 slots
            INVARIANT(s.partials == s.wpo && s.grid * 256 >= n * s.wpo * 64 && s.scal < 0);
            INVARIANT(p.naf == (p.n_stages == 1 ? 2 : 1) && n <= p.t3_points);                // the only stage folds 1/n in; every input has its x3 tables
            break;
        case G1S_FIRST_TABLES:
            INVARIANT(i == 0 && !planes && p.tab_W > 0 && p.tab_c > 0 && (size_t)s.wpo * 32 >= R * p.tab_W && s.partials == s.wpo && s.grid * 256 >= n * s.wpo * 64);
            INVARIANT(s.scal == (G1SCAL_CANON | (p.n_stages == 1 ? G1SCAL_SCALED : 0)));
            break;
        case G1S_DIRECT: case G1S_DIRECT_PAIRS:
            INVARIANT(s.K >= 1 && s.K <= 5);                                                   // the in-wave tree: R <= 32 terms of an output in one wave
            INVARIANT(s.grid * 256 >= (n << s.K) * LANES_PER_POINT[s.kind] && !s.partials);
            break;
        case G1S_MUL_QUADS:
            INVARIANT(s.K >= 1 && s.K <= 5 && s.partials == R && s.grid * 256 >= (n << s.K) * 4);
            break;
        case G1S_RADIX2: case G1S_RADIX2_PAIRS:
            INVARIANT(s.K == 1 && s.log_s == i && s.src == s.dst && s.grid * 256 >= n / 2 * LANES_PER_POINT[s.kind] && !s.partials);
            INVARIANT(s.kind == G1S_RADIX2 || n / 2 >= 32);                                    // k_g1fft_stage_pairs: whole waves are active or not, except the last
            break;
        default: INVARIANT(!"a stage kind");
        }
        if (s.kind == G1S_DIRECT || s.kind == G1S_DIRECT_PAIRS || s.kind == G1S_MUL_QUADS) {
            int done = 0;
            for (int k = 0; k <= i; ++k) done += p.stage[k].K;
            INVARIANT(s.log_s == p.log_n - done);
        }
        INVARIANT(!s.last || i == p.n_stages - 1);
    }
    INVARIANT(bits_sum == p.log_n);                                                            // the stages' K sum to log n
    INVARIANT(holds == p.result);
    INVARIANT(p.t3 == (bits_stages > 0) && (p.naf != 0) == p.t3 && (p.t3_points != 0) == p.t3);  // the x3 tables exactly when a bits stage exists
    if (planes) {
        INVARIANT(p.bytes_a == 0 && p.bytes_b == 0 && p.bytes_c == 0 && max_partial_points == 0);
    } else {
        INVARIANT(p.bytes_c >= max_partial_points * G1FFT_POINT_BYTES);                       // .c holds the largest partial array of any stage
        INVARIANT(p.bytes_b >= 2 * n * G1FFT_POINT_BYTES && p.bytes_a >= n * 9 * 4);          // .b two plane sets, .a nine limb planes of prefix products
    }
}

int main() {
    g1fft_grid(
        [&](const G1fftSrsCase& c, int log_n) {
            snprintf(case_name, sizeof case_name, "ifft %s log_n=%d", c.name, log_n);
            G1fftSrsShape srs;
            srs.n = g1fft_case_srs_n(c, log_n); srs.monomial = !c.lagrange; srs.bit_tables = c.bits;
            srs.small_c = c.small_c; srs.small_W = c.small_W; srs.pre_c = c.pre_c; srs.pre_W = c.pre_W;
            const G1fftPlan p = g1fft_plan_ifft((size_t)1 << log_n, srs);
            static const char* const names[3] = {"srs", "A", "B"};
            g1fft_print_ifft_case(c, log_n);
            print_plan(p, names);
            check_invariants(p, false);
        },
        [&](int log_n, bool inverse, bool scaled, bool strided) {
            snprintf(case_name, sizeof case_name, "planes log_n=%d inverse=%d scaled=%d strided=%d", log_n, (int)inverse, (int)scaled, (int)strided);
            const G1fftPlan p = g1fft_plan_planes((size_t)1 << log_n, inverse, scaled, strided);
            const char* const names[3] = {"in", p.result ? "tmp" : "out", p.result ? "out" : "tmp"};      // the caller's rule: buffer `result` is out
            g1fft_print_planes_case(log_n, inverse, scaled, strided);
            print_plan(p, names);
            check_invariants(p, true);
            INVARIANT(strcmp(names[1 + p.result], "out") == 0);
            for (int i = 0; i < p.n_stages; ++i) INVARIANT((p.stage[i].scal >= 0) == (p.stage[i].K > 0) && (p.stage[i].scal < 0 || ((p.stage[i].scal & G1SCAL_FORWARD) != 0) == !inverse));
        });
    if (failures) fprintf(stderr, "g1fft_plancheck: %d invariant(s) violated\n", failures);
    return failures ? 1 : 0;
}
