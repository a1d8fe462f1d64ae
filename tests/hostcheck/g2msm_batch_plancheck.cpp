// tests/hostcheck/g2msm_batch_plancheck.cpp — TEST-ONLY driver for a plain g++ build (no GPU, no library) of the BATCH planner of
// csrc/g2msm_plan.h (g2_batch_group, g2_make_batch_plan, g2_batch_plan_status): every n in 1 .. 2^20 that is a power of two or one beside
// it, nb in {1, 2}, the blob counts and caps below; one line per plan on stdout, a line on stderr and exit status 1 per violated
// invariant.  Built and run by tests/test_g2msm_batch_plan_host.py, which also reads the lines for the paths the grid must cover.
#include <cstdio>
#include <set>
#include <vector>

#include "g2msm_plan.h"

using namespace kzg;

static constexpr uint32_t WAVE_SLOTS = 256 * 4 * G2_ACC_WAVES;        // a 256-CU device

static int failures = 0;
#define G2B_INVARIANT(c) do { if (!(c)) { ++failures; fprintf(stderr, "g2msm_batch_plancheck: n=%zu nb=%u count=%zu max=%u: %s\n", n, nb, count, max_blobs, #c); } } while (0)

// the three caps of a group, as the issue of the batched call states them
static size_t windows(size_t n) { const int c = generic_window(n, 1); return (size_t)(255 + c - 1) / c; }
static bool results_fit(size_t n, uint32_t nb, size_t blobs) { return nb * windows(n) * blobs <= (size_t)MSM_MAX_OUT * 32 / G2_WIRE_WORDS; }
static bool entries_fit(size_t n, size_t blobs) { return windows(n) * n * blobs <= ((size_t)1 << 27); }
static bool scan_fits(size_t n, size_t blobs) {
    const size_t G = blobs * windows(n) << (generic_window(n, 1) - 1);
    return G <= SCAN1_MAX || (G + SCAN_TILE - 1) / SCAN_TILE <= (size_t)SCAN_TILE;
}
static bool caps_hold(size_t n, uint32_t nb, size_t blobs) { return results_fit(n, nb, blobs) && entries_fit(n, blobs) && scan_fits(n, blobs); }

int main() {
    std::set<size_t> ns;
    const size_t top = (size_t)1 << 20;
    for (size_t p = 1; p <= top; p *= 2) { if (p > 1) ns.insert(p - 1); ns.insert(p); if (p < top) ns.insert(p + 1); }
    const size_t counts[] = {1, 2, 3, 5, 16, 64, 95, 96, 1024};
    const size_t point = 72 * 4;
    for (uint32_t nb = 1; nb <= 2; ++nb)
        for (size_t n : ns)
            for (size_t count : counts)
                for (uint32_t max_blobs : {0u, 2u}) {
                    const uint32_t group = g2_batch_group(n, nb, count, max_blobs);
                    // batched = 0 exactly when the rule says so: a blob above one launch, or no group of two fits
                    const bool want_batched = n <= G2MSM_MAX_LAUNCH && caps_hold(n, nb, 2);
                    G2B_INVARIANT((group != 0) == want_batched);
                    if (!group) { printf("n=%zu nb=%u count=%zu max=%u batched=0\n", n, nb, count, max_blobs); continue; }
                    // the group: all three caps hold; one more blob would break one of them, or pass max_blobs, or the count
                    G2B_INVARIANT(group >= 1 && group <= count && (!max_blobs || group <= max_blobs) && caps_hold(n, nb, group));
                    const bool result_binds = !results_fit(n, nb, group + 1), entry_binds = !entries_fit(n, group + 1);
                    G2B_INVARIANT(!caps_hold(n, nb, group + 1) || group == count || (max_blobs && group == max_blobs));
                    const G2BatchPlan p = g2_make_batch_plan(n, nb, group, WAVE_SLOTS);
                    const char* error = nullptr;
                    G2B_INVARIANT(g2_batch_plan_status(p, n, G2_RESULT_CAP, &error) == KZG_OK && error == nullptr);
                    G2B_INVARIANT(p.c == generic_window(n, 1) && p.W == (255 + p.c - 1) / p.c && p.B == (1u << (p.c - 1)) && p.G == group * (uint32_t)p.W * p.B);
                    G2B_INVARIANT(p.blobs == group && p.n_windows() == group * (uint32_t)p.W && p.entries() == (size_t)group * p.W * n);
                    // lanes: whole workgroups, one round of resident waves at most, every entry covered, at most four lanes per bucket
                    G2B_INVARIANT(p.nl % 256 == 0 && p.nl >= 256 && p.nl <= WAVE_SLOTS * 64);
                    G2B_INVARIANT((size_t)p.seg * p.nl >= p.entries() && (size_t)(p.seg - 1) * p.nl < p.entries());
                    G2B_INVARIANT(p.nl <= std::max<size_t>(256, ((size_t)4 * p.G + 255) / 256 * 256));
                    G2B_INVARIANT(p.T * p.m == p.B && p.T >= 2 && p.T <= G2_RED_T && (p.T & (p.T - 1)) == 0);
                    // every buffer is as large as the kernels index it (g2msm.hip g2_msm_batch_launch)
                    G2B_INVARIANT(p.bytes[G2WS_HEAD] >= (size_t)nb * p.G * point && p.bytes[G2WS_BUCKET] >= (size_t)nb * p.G * point);
                    G2B_INVARIANT(p.bytes[G2WS_CONT] >= (size_t)nb * p.nl * point);
                    G2B_INVARIANT(p.n_chunks() == group * (uint32_t)p.W * p.T);
                    for (int b : {G2WS_CHUNK_S, G2WS_CHUNK_TMP, G2WS_CHUNK_A}) G2B_INVARIANT(p.bytes[b] >= (size_t)nb * group * p.W * p.T * point);
                    G2B_INVARIANT(p.n_out == nb * group * (uint32_t)p.W && p.n_out <= G2_RESULT_CAP);
                    // the sort: the generic one over `group` sets of n scalars, in-blob indices, buffers for every entry and bucket
                    G2B_INVARIANT(p.sort.shared_bases && !p.sort.tables && !p.sort.sort2 && !p.sort.lean_sort && p.sort.batch == group && p.sort.n == p.n &&
                                  p.sort.c == p.c && p.sort.G == p.G && p.sort.set_len == p.n && p.sort.sets == group * (uint32_t)p.W);
                    G2B_INVARIANT(p.sort.bytes[WS_SORTED] >= p.entries() * 4 && p.sort.bytes[WS_DIGITS] >= p.entries() * 4);
                    G2B_INVARIANT(p.sort.bytes[WS_COUNT] >= (size_t)p.G * 4 && p.sort.bytes[WS_OFFS] >= ((size_t)p.G + 1) * 4);
                    G2B_INVARIANT(p.sort.bytes[WS_BLOCKBASE] >= (p.sort.sort_small ? (size_t)p.G * 4 : (size_t)p.sort.tiles * p.B * 4));
                    G2B_INVARIANT(p.sort.sort_small || (size_t)p.B * 4 <= SORT1_MAX_LDS);
                    G2B_INVARIANT(p.entries() <= ((size_t)1 << 27));                      // 32-bit positions, the sign bit of an entry free
                    G2B_INVARIANT(p.launches == 2u + (p.sort.sort_small ? 1u : 0u) + 1u + (p.G <= SCAN1_MAX ? 1u : 3u) + 1u + 6u);
                    printf("n=%zu nb=%u count=%zu max=%u batched=1 group=%u c=%d W=%d G=%u entries=%zu nl=%u seg=%u small=%d scan1=%d launches=%u bytes=%zu result_binds=%d entry_binds=%d\n",
                           n, nb, count, max_blobs, group, p.c, p.W, p.G, p.entries(), p.nl, p.seg, (int)p.sort.sort_small, (int)(p.G <= SCAN1_MAX), p.launches,
                           p.workspace_bytes, (int)result_binds, (int)entry_binds);
                }
    // rejections
    {
        const size_t n = 16, count = 0; const uint32_t nb = 1, max_blobs = 0;
        const char* error = nullptr;
        G2B_INVARIANT(g2_batch_group((size_t)G2MSM_MAX_LAUNCH + 1, 1, 64, 0) == 0);          // above one launch: blob by blob
        G2B_INVARIANT(g2_batch_group(0, 1, 64, 0) == 0 && g2_batch_group(16, 3, 64, 0) == 0);
        G2B_INVARIANT(g2_batch_plan_status(g2_make_batch_plan(0, 1, 2, WAVE_SLOTS), 0, G2_RESULT_CAP, &error) == KZG_ERR_INVALID_ARG);
        G2B_INVARIANT(g2_batch_plan_status(g2_make_batch_plan(16, 3, 2, WAVE_SLOTS), 16, G2_RESULT_CAP, &error) == KZG_ERR_INVALID_ARG);
        G2B_INVARIANT(g2_batch_plan_status(g2_make_batch_plan(16, 1, 0, WAVE_SLOTS), 16, G2_RESULT_CAP, &error) == KZG_ERR_INVALID_ARG);
        G2B_INVARIANT(g2_batch_plan_status(g2_make_batch_plan(4096, 2, 96, WAVE_SLOTS), 4096, G2_RESULT_CAP, &error) == KZG_ERR_INVALID_ARG && error);    // 8 256 result values
        G2B_INVARIANT(g2_batch_plan_status(g2_make_batch_plan((size_t)1 << 20, 1, 7, WAVE_SLOTS), (size_t)1 << 20, G2_RESULT_CAP, &error) == KZG_ERR_INVALID_ARG && error);   // 19 x 7 x 2^20 entries
        G2B_INVARIANT(g2_batch_plan_status(g2_make_batch_plan(4096, 2, 95, WAVE_SLOTS), 4096, G2_RESULT_CAP, &error) == KZG_OK);
    }
    return failures ? 1 : 0;
}
