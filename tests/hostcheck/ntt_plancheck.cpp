// tests/hostcheck/ntt_plancheck.cpp — TEST-ONLY driver for a plain g++ build (no GPU, no library) of csrc/ntt_plan.h: prints the plan of every
// case of the fixed grid (ntt_grid.h) in the format of tests/golden/ntt_plans.txt and checks, on every plan, what k_ntt_pass and ntt_run rely on
// whatever the policy decides.  Built and run by tests/test_ntt_plan_host.py and, under ASan + UBSan, by tests/test_sanitizers_host.py.  Exit
// status 1 and a line on stderr per violated invariant.
#include <cstdio>

#include "ntt_plan.h"
#include "ntt_grid.h"

using namespace kzg;

static int failures = 0;
static char case_name[96];
#define INVARIANT(c) do { if (!(c)) { ++failures; fprintf(stderr, "ntt_plancheck: %s: %s\n", case_name, #c); } } while (0)

static const int TILE_LOG[NTT_KERNELS] = {11, 10, 10, 10, 10}, KMAX_T[NTT_KERNELS] = {10, 10, 7, 8, 9}, PER_CU[NTT_KERNELS] = {1, 2, 3, 3, 3};
static const char* const BUF[3] = {"caller", "data", "tmp"};

static void check_invariants(const NttPlan& p, int cus, bool tw_arrays) {
    const size_t n = (size_t)1 << p.log_n;
    INVARIANT(p.n_passes >= 1 && p.n_passes <= NTT_MAX_PASSES && p.kernel >= 0 && p.kernel < NTT_KERNELS);
    INVARIANT(p.threads == (1 << TILE_LOG[p.kernel]) / NTT_EPT);
    INVARIANT(p.bytes_data == (p.n_passes > 1 ? n * 32 : 0) && p.bytes_tmp == (p.n_passes > 2 ? n * 32 : 0));      // tmp is reserved exactly when P > 2
    int bits = 0, holds = NTT_BUF_CALLER, folds = 0;
    for (int i = 0; i < p.n_passes; ++i) {
        const NttPass& s = p.pass[i];
        const NttPassArgs& a = s.args;
        const bool last = i == p.n_passes - 1;
        bits += a.K;
        INVARIANT(a.K >= 1 && a.K <= NTT_KMAX && a.K <= KMAX_T[p.kernel] && a.K <= TILE_LOG[p.kernel]);     // a slim instantiation only with every K <= its bound
        INVARIANT(a.log_n == p.log_n && a.log_s == p.log_n - bits);
        INVARIANT(last ? a.next_K == 0 && a.next_log_s == 0 : a.next_K == p.pass[i + 1].args.K && a.next_log_s == p.log_n - bits - a.next_K);
        INVARIANT(s.src == holds);                                                                      // each pass reads what the one before wrote
        INVARIANT(last ? s.dst == NTT_BUF_CALLER : (s.dst == NTT_BUF_DATA || s.dst == NTT_BUF_TMP) && s.dst != s.src);
        INVARIANT(s.dst != NTT_BUF_DATA || p.bytes_data);
        INVARIANT(s.dst != NTT_BUF_TMP || p.bytes_tmp);
        holds = s.dst;
        const uint32_t units = (uint32_t)(n >> a.K), C = 1u << (TILE_LOG[p.kernel] - a.K);
        INVARIANT(a.n_tiles == (units + C - 1) / C && a.n_tiles >= 1);
        INVARIANT(s.grid >= 1 && s.grid <= a.n_tiles && s.grid <= (uint32_t)(cus * PER_CU[p.kernel]) && (s.grid == a.n_tiles || s.grid == (uint32_t)(cus * PER_CU[p.kernel])));
        INVARIANT(s.tw == (!last && p.log_n <= NTT_FULL_TW_MAX_LOG));                                    // an array exactly when the pass is not last and log n <= 22
        INVARIANT(!s.tw_scaled || (s.tw && p.inverse && i == p.n_passes - 2));
        folds += s.tw_scaled;
        INVARIANT(a.scale_log_n == -1 || (last && p.inverse && a.scale_log_n == p.log_n));
    }
    INVARIANT(bits == p.log_n && holds == NTT_BUF_CALLER);                                              // the K sum to log n; the last pass writes the caller's data
    INVARIANT(folds <= 1 && (!folds || p.inverse));                                                     // at most one boundary folds the scale, on an inverse transform
    // exactly one place scales an inverse transform, none a forward one
    const int last_scales = p.pass[p.n_passes - 1].args.scale_log_n >= 0;
    INVARIANT(last_scales + (folds && tw_arrays ? 1 : 0) == (p.inverse ? 1 : 0));
}

int main() {
    int cases = 0;
    ntt_grid([&](int log_n, bool inverse, int tile_env, int cus, bool tw_arrays) {
        ++cases;
        snprintf(case_name, sizeof case_name, "log_n=%d inverse=%d tile_env=%d cus=%d tw_arrays=%d", log_n, (int)inverse, tile_env, cus, (int)tw_arrays);
        NttPlan p = ntt_plan(log_n, inverse, cus, tile_env);
        for (int i = 0; i < p.n_passes; ++i)                       // the driver's half of the rule: the fetch of the scaled array returned none
            if (p.pass[i].tw_scaled && !tw_arrays) ntt_plan_fold_missing(p);
        ntt_print_case(log_n, inverse, tile_env, cus, tw_arrays);
        ntt_print_plan(TILE_LOG[p.kernel], KMAX_T[p.kernel], p.threads, p.n_passes, p.bytes_data, p.bytes_tmp);
        for (int i = 0; i < p.n_passes; ++i) {
            const NttPass& s = p.pass[i];
            ntt_print_pass(s.args.K, s.args.log_s, s.args.next_K, s.args.next_log_s, s.args.scale_log_n, s.args.n_tiles, s.grid, BUF[s.src], BUF[s.dst],
                           !s.tw ? "-" : s.tw_scaled ? "scaled" : "plain", s.tw && tw_arrays);
        }
        ntt_end_case();
        check_invariants(p, cus, tw_arrays);
    });
    ntt_end_table();
    INVARIANT(cases == NTT_GRID_CASES);
    if (failures) fprintf(stderr, "ntt_plancheck: %d invariant(s) violated\n", failures);
    return failures ? 1 : 0;
}
