// tests/hostcheck/plancheck.cpp — TEST-ONLY driver for a plain g++ build (no GPU, no library) of csrc/msm_plan.h: prints the plan of every
// case of the fixed grid (plan_grid.h) in the format of tests/golden/msm_plans.txt and checks, on every accepted plan, what must hold
// whatever the policy decides: the grid shapes the kernels assume and that every workspace buffer is as large as the chosen kernels index
// it (read off their launch arguments in msm.hip).  Built and run by tests/test_msm_plan_host.py and, under ASan + UBSan, by
// tests/test_sanitizers_host.py.  Exit status 1 and a line on stderr per violated invariant.
#include <cstdio>

#include "msm_plan.h"
#include "plan_grid.h"

using namespace kzg;

static int failures = 0;
#define INVARIANT(c) do { if (!(c)) { ++failures; fprintf(stderr, "plancheck: case %d (%s n=%zu batch=%u polys=%u): %s\n", case_no, g.bases, g.n, g.batch, g.polys, #c); } } while (0)

static void check_invariants(int case_no, const GridCase& g, const Plan& p) {
    const size_t plane = 36 * 4;                     // one XYZZ value in limb planes
    if (p.bitsum) {
        INVARIANT(p.bitsum_chunk == 8 || p.bitsum_chunk == 16 || p.bitsum_chunk == 32);
        INVARIANT((size_t)p.bitsum_wg * 64 >= (size_t)p.n * (256 / p.bitsum_chunk));           // one quad per (scalar, chunk of positions)
        INVARIANT(p.bytes[WS_CHUNK_S] >= (size_t)p.bitsum_wg * plane);
        INVARIANT((size_t)p.n_out * 64 >= p.bitsum_wg && p.n_out <= 8 * (g.n > 4096 ? 2u : 1u));
        return;
    }
    const size_t entries = p.entries();
    INVARIANT(p.nl % 256 == 0 && p.nl >= 256 && p.nl <= (1u << 24));
    INVARIANT((size_t)p.tiles_per_set * p.tile_len >= p.set_len);
    INVARIANT(p.tiles == p.tiles_per_set * p.sets && p.G == p.sets * p.B);
    // exactly one sort form: two-level | lean | global-atomic | single-pass tiled
    const bool tiled = !p.sort2 && !p.sort_small;
    INVARIANT((int)p.sort2 + (int)p.lean_sort + (int)(p.sort_small && !p.lean_sort) + (int)tiled == 1);
    INVARIANT(!p.lean_sort || (p.sort_small && p.tables && p.G <= SCAN1_MAX));
    INVARIANT(!tiled || (size_t)p.B * 4 <= SORT1_MAX_LDS);                                      // one LDS counter per bucket
    INVARIANT(!p.polys || p.B % 128 == 0);
    INVARIANT(!p.fused || (p.tables && !p.naf));
    INVARIANT(p.T * p.m == p.B && p.T <= (uint32_t)RED_T);
    INVARIANT(p.G <= SCAN1_MAX || p.scan_blocks() <= (uint32_t)SCAN_TILE);
    // workspace: sort
    INVARIANT(p.bytes[WS_SORTED] >= entries * 4);
    INVARIANT(p.bytes[WS_COUNT] >= (size_t)p.G * 4 && p.bytes[WS_OFFS] >= ((size_t)p.G + 1) * 4);
    INVARIANT(p.G <= SCAN1_MAX || p.bytes[WS_BLOCK_SUMS] >= (size_t)p.scan_blocks() * 4);
    if (p.sort2) {
        INVARIANT(p.Hb == p.B >> SORT2_LO_BITS && p.Hb >= 1 && p.Hb <= SORT2_MAX_BINS);
        INVARIANT((size_t)p.tiles1 * p.tile1 >= p.n);
        INVARIANT((size_t)p.tiles2cap >= entries / SORT2_CHUNK + p.Hb);                         // tiles of LARGE bins: one partial tile per bin at most
        INVARIANT(p.bytes[WS_SORT_TMP] >= entries * 4);
        INVARIANT(p.bytes[WS_SORT_SMALL] >= ((size_t)3 * (p.Hb + 1) + p.tiles2cap + 1) * 4);    // ccount | cstart | tstart | tile_bin | bin_cap
        INVARIANT(p.bytes[WS_BLOCKBASE] >= (size_t)p.tiles1 * p.Hb * 4 && p.bytes[WS_BLOCKBASE] >= (size_t)p.tiles2cap * SORT2_LO * 4);
        if (p.naf) {
            INVARIANT(p.ND == 32 || p.ND == NAF_DIGITS);
            INVARIANT(p.W <= p.ND && p.W == naf_max_digits(p.c + 1));                           // every digit of a scalar has a word
            INVARIANT(p.bytes[WS_SORT_KEY] >= entries && p.bytes[WS_DIGITS] >= (size_t)p.n * p.ND * 4);
            INVARIANT(((size_t)3 * p.Hb + (size_t)SORT2_P1_THREADS * p.W) * 4 + (size_t)SORT2_P1_THREADS * p.W * 2 <=
                      ((size_t)3 * SORT2_MAX_BINS + (size_t)SORT2_P1_THREADS * (p.ND == 32 ? 32 : 31)) * 4 + (size_t)SORT2_P1_THREADS * (p.ND == 32 ? 32 : 31) * 2);
        } else {
            INVARIANT((size_t)p.W * p.idx_stride <= ((size_t)1 << SORT2_IDX_BITS));             // the index field of an entry between the passes
        }
    } else {
        INVARIANT(p.bytes[WS_DIGITS] >= entries * 4);
        INVARIANT(p.bytes[WS_BLOCKBASE] >= (p.sort_small ? (size_t)p.G * 4 : (size_t)p.tiles * p.B * 4));
    }
    if (p.idx_log != 31) INVARIANT((1u << p.idx_log) == p.idx_stride && p.idx_stride >= p.n && p.idx_stride + p.stride_adj == g.stride);
    // workspace: accumulate and reduction
    INVARIANT(p.bytes[WS_HEAD] >= (size_t)p.G * plane && p.bytes[WS_CONT] >= (size_t)p.nl * plane);
    if (p.tables) {
        INVARIANT(p.sets == 1 && p.batch == 1 && p.B % 64 == 0);
        INVARIANT(p.bytes[WS_CHUNK_S] >= (size_t)7 * p.G1() * plane);
        INVARIANT(p.n_out == (p.polys && p.c == 7 ? p.polys : p.G1() == 1 ? 7 : 13 * p.G1p()));
        INVARIANT(!p.quad1 || p.quad);
        if (p.polys && p.c == 7) INVARIANT(p.G1() >= p.polys);                                  // one group of 64 buckets per polynomial
        if (p.polys && p.c != 7) INVARIANT(p.G1p() == p.polys * ((1u << (p.c - 1)) / 4096u));   // whole units per polynomial
    } else {
        INVARIANT(p.sets == p.n_windows() && p.n_out == p.n_windows());
        INVARIANT(p.bytes[WS_BUCKET] >= (size_t)p.G * plane);
        INVARIANT(p.bytes[WS_CHUNK_S] >= (size_t)p.n_chunks() * plane && p.bytes[WS_CHUNK_TMP] >= (size_t)p.n_chunks() * plane &&
                  p.bytes[WS_CHUNK_A] >= (size_t)p.n_chunks() * plane);
    }
    INVARIANT(p.n_out <= g.out_cap && g.out_off + p.n_out <= MSM_MAX_OUT);
}

int main() {
    int case_no = 0;
    plan_grid([&](const GridCase& g) {
        ++case_no;
        PlanContext ctx;
        ctx.msm_c_override = g.c_over; ctx.msm_seg_override = g.seg_over; ctx.reduction_lanes = g.lanes; ctx.acc_wave_slots = g.wave_slots;
        ctx.other_in_flight = !g.alone;
        MsmBasesShape bases;
        bases.table_stride = g.stride; bases.c = g.c; bases.W = g.W; bases.naf = g.naf; bases.bitsum = g.bitsum;
        const Plan p = make_plan(ctx, g.n, bases, g.batch, g.polys);
        const char* error = nullptr;
        const int32_t status = msm_plan_status(p, bases, g.polys, g.out_off, g.out_cap, &error);
        if (status != KZG_OK) return print_rejected(g, status, error);
        print_plan(g, p, p.fused, p.ND, p.lean_sort, p.quad1, p.n_out);
        if (p.bitsum) printf("    bitsum chunk=%d n_wg=%u\n", p.bitsum_chunk, p.bitsum_wg);
        check_invariants(case_no, g, p);
    });
    plan_grid_sizes([](uint32_t stride, int W, bool naf) { MsmBasesShape b; b.table_stride = stride; b.W = W; b.naf = naf; return msm_launch_len(b); },
                    [](size_t len) { return msm_batch_capacity(len); });
    if (failures) fprintf(stderr, "plancheck: %d invariant(s) violated\n", failures);
    return failures ? 1 : 0;
}
