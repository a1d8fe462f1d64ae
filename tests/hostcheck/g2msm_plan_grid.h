// tests/hostcheck/g2msm_plan_grid.h — the cases and invariants of the G2 MSM planner (csrc/g2msm_plan.h: g2_batch_group, g2_make_plan,
// g2_plan_status), shared by g2msm_plancheck.cpp and the sanitizer program g2_sanitize_main.cpp: every n in 1 .. 2^20 that is a power of
// two or one beside it, and every n at which the plan of one blob changes shape (window bits, sort form, scan form, saturated lanes) with
// its two neighbours; over that nb in {1, 2}, the blob counts and the caller's caps below.
#pragma once
#include <cstdio>
#include <set>
#include <vector>

#include "g2msm_plan.h"

namespace g2grid {
using namespace kzg;

constexpr uint32_t WAVE_SLOTS = 256 * 4 * G2_ACC_WAVES;        // a 256-CU device

// whether the G2_SEG_MIN share of the entries fills one round of resident waves (whole workgroups), whatever the bucket cap then does
inline bool share_fills_chip(const G2Plan& p) { return ((p.entries() + G2_SEG_MIN - 1) / G2_SEG_MIN + 255) / 256 * 256 >= (size_t)WAVE_SLOTS * 64; }
// the fields that make a plan's SHAPE: which kernels run and how the buffers are indexed, not how large they are
inline bool same_shape(const G2Plan& a, const G2Plan& b) {
    return a.c == b.c && a.W == b.W && a.B == b.B && a.T == b.T && a.m == b.m && a.sort.sort_small == b.sort.sort_small &&
           (a.G <= SCAN1_MAX) == (b.G <= SCAN1_MAX) && (a.nl == WAVE_SLOTS * 64) == (b.nl == WAVE_SLOTS * 64) &&
           share_fills_chip(a) == share_fills_chip(b) && a.launches == b.launches;
}
inline std::vector<size_t> cases() {
    std::set<size_t> ns;
    const size_t top = (size_t)1 << 20;
    for (size_t p = 1; p <= top; p *= 2) { if (p > 1) ns.insert(p - 1); ns.insert(p); if (p < top) ns.insert(p + 1); }
    // shape boundaries by bisection between consecutive powers of two (a shape changes at most a few times in between)
    for (size_t lo = 1; lo < top; lo *= 2) {
        std::vector<std::pair<size_t, size_t>> todo = {{lo, lo * 2}};
        while (!todo.empty()) {
            auto [a, b] = todo.back();
            todo.pop_back();
            if (b - a <= 1 || same_shape(g2_make_plan(a, 1, 1, WAVE_SLOTS), g2_make_plan(b, 1, 1, WAVE_SLOTS))) {
                if (b - a == 1 && !same_shape(g2_make_plan(a, 1, 1, WAVE_SLOTS), g2_make_plan(b, 1, 1, WAVE_SLOTS))) { ns.insert(a); ns.insert(b); }
                continue;
            }
            const size_t mid = a + (b - a) / 2;
            todo.push_back({a, mid});
            todo.push_back({mid, b});
        }
    }
    return std::vector<size_t>(ns.begin(), ns.end());
}

// the three caps of a group, as the issue of the batched call states them
inline size_t windows(size_t n) { const int c = generic_window(n, 1); return (size_t)(255 + c - 1) / c; }
inline bool results_fit(size_t n, uint32_t nb, size_t blobs) { return nb * windows(n) * blobs <= (size_t)MSM_MAX_OUT * 32 / G2_WIRE_WORDS; }
inline bool entries_fit(size_t n, size_t blobs) { return windows(n) * n * blobs <= ((size_t)1 << 27); }
inline bool scan_fits(size_t n, size_t blobs) {
    const size_t G = blobs * windows(n) << (generic_window(n, 1) - 1);
    return G <= SCAN1_MAX || (G + SCAN_TILE - 1) / SCAN_TILE <= (size_t)SCAN_TILE;
}
inline bool caps_hold(size_t n, uint32_t nb, size_t blobs) { return results_fit(n, nb, blobs) && entries_fit(n, blobs) && scan_fits(n, blobs); }
// the lane rule, restated: one round of resident waves, G2_SEG_MIN entries per lane, four lanes per bucket -- the least of the three, in
// whole workgroups, one workgroup at least
inline size_t lanes_rule(size_t E, size_t G) {
    size_t l = (size_t)64 * (WAVE_SLOTS > 4 ? WAVE_SLOTS : 4);
    if ((E + 3) / 4 < l) l = (E + 3) / 4;
    if (4 * G < l) l = 4 * G;
    l = (l + 255) / 256 * 256;
    return l < 256 ? 256 : l;
}

#define G2_INVARIANT(c) do { if (!(c)) { ++failures; fprintf(stderr, "g2msm_plancheck: n=%zu nb=%u count=%zu max=%u: %s\n", n, nb, count, max_blobs, #c); } } while (0)

// the invariants of one plan; `group` blobs of n scalars
inline int check_plan(const G2Plan& p, size_t n, uint32_t nb, size_t count, uint32_t max_blobs, uint32_t group) {
    int failures = 0;
    const size_t point = 72 * 4;
    const char* error = nullptr;
    G2_INVARIANT(g2_plan_status(p, n, G2_RESULT_CAP, &error) == KZG_OK && error == nullptr);       // every plan of the grid passes its own status function
    G2_INVARIANT(G2_RESULT_CAP == MSM_MAX_OUT * 32 / G2_WIRE_WORDS);
    G2_INVARIANT(p.c == generic_window(n, 1) && p.W == (255 + p.c - 1) / p.c && p.B == (1u << (p.c - 1)) && p.G == group * (uint32_t)p.W * p.B);
    G2_INVARIANT(p.blobs == group && p.n_windows() == group * (uint32_t)p.W && p.entries() == (size_t)group * p.W * n);
    // lanes: whole workgroups, one round of resident waves at most, every entry covered by the equal share, the lane rule exactly
    G2_INVARIANT(p.nl % 256 == 0 && p.nl >= 256 && p.nl <= WAVE_SLOTS * 64);
    G2_INVARIANT((size_t)p.seg * p.nl >= p.entries() && (size_t)(p.seg - 1) * p.nl < p.entries());
    G2_INVARIANT(p.nl == lanes_rule(p.entries(), p.G));
    G2_INVARIANT(p.seg == (p.entries() + p.nl - 1) / p.nl);
    G2_INVARIANT(p.nl <= std::max<size_t>(256, ((size_t)4 * p.G + 255) / 256 * 256));
    G2_INVARIANT(p.fin_adds_bound() <= WAVE_SLOTS + 7);                   // bucket kernel: the partials of one bucket over the 64 lanes of a wave
    G2_INVARIANT(p.T * p.m == p.B && p.T >= 2 && p.T <= G2_RED_T && (p.T & (p.T - 1)) == 0);
    // every buffer is as large as the kernels index it (g2msm.hip g2_msm_launch)
    G2_INVARIANT(p.bytes[G2WS_HEAD] >= (size_t)nb * p.G * point && p.bytes[G2WS_BUCKET] >= (size_t)nb * p.G * point);
    G2_INVARIANT(p.bytes[G2WS_CONT] >= (size_t)nb * p.nl * point);
    G2_INVARIANT(p.n_chunks() == group * (uint32_t)p.W * p.T);
    for (int b : {G2WS_CHUNK_S, G2WS_CHUNK_TMP, G2WS_CHUNK_A}) G2_INVARIANT(p.bytes[b] >= (size_t)nb * group * p.W * p.T * point);
    G2_INVARIANT(p.n_out == nb * group * (uint32_t)p.W && p.n_out <= G2_RESULT_CAP && p.n_out * G2_WIRE_WORDS <= MSM_MAX_OUT * 32);
    // the sort: the generic one over `group` sets of n scalars, in-blob indices, buffers for every entry and bucket
    G2_INVARIANT(p.sort.shared_bases && !p.sort.tables && !p.sort.sort2 && !p.sort.lean_sort && p.sort.batch == group && p.sort.n == p.n &&
                 p.sort.c == p.c && p.sort.G == p.G && p.sort.set_len == p.n && p.sort.sets == group * (uint32_t)p.W);
    G2_INVARIANT(p.sort.bytes[WS_SORTED] >= p.entries() * 4 && p.sort.bytes[WS_DIGITS] >= p.entries() * 4);
    G2_INVARIANT(p.sort.bytes[WS_COUNT] >= (size_t)p.G * 4 && p.sort.bytes[WS_OFFS] >= ((size_t)p.G + 1) * 4);
    G2_INVARIANT(p.sort.bytes[WS_BLOCKBASE] >= (p.sort.sort_small ? (size_t)p.G * 4 : (size_t)p.sort.tiles * p.B * 4));
    G2_INVARIANT(p.sort.sort_small || (size_t)p.B * 4 <= SORT1_MAX_LDS);
    G2_INVARIANT(p.entries() <= ((size_t)1 << 27));                       // 32-bit positions, the sign bit of an entry free
    G2_INVARIANT(p.launches == 2u + (p.sort.sort_small ? 1u : 0u) + 1u + (p.G <= SCAN1_MAX ? 1u : 3u) + 1u + 6u);
    return failures;
}

// Prints to `out` (may be null) one line per plan of one blob ("n=.. nb=.. c=..": the single call), then one line per (n, nb, count,
// max_blobs) of the grid ("n=.. nb=.. count=..": the group of that call); returns the number of violated invariants.
inline int run(FILE* out) {
    int failures = 0;
    const std::vector<size_t> ns = cases();
    const size_t counts[] = {1, 2, 3, 5, 16, 64, 95, 96, 1024};
    for (uint32_t nb = 1; nb <= 2; ++nb) {
        G2Plan prev{};
        bool have_prev = false;
        for (size_t n : ns) {
            const size_t count = 1; const uint32_t max_blobs = 0;
            const G2Plan p = g2_make_plan(n, nb, 1, WAVE_SLOTS);
            failures += check_plan(p, n, nb, count, max_blobs, 1);
            if (have_prev && same_shape(prev, p)) G2_INVARIANT(p.workspace_bytes >= prev.workspace_bytes);      // monotone within a shape
            if (out)
                fprintf(out, "n=%zu nb=%u c=%d W=%d B=%u nl=%u seg=%u T=%u m=%u small=%d scan1=%d launches=%u n_out=%u bytes=%zu\n", n, nb, p.c, p.W, p.B, p.nl,
                        p.seg, p.T, p.m, (int)p.sort.sort_small, (int)(p.G <= SCAN1_MAX), p.launches, p.n_out, p.workspace_bytes);
            prev = p;
            have_prev = true;
        }
    }
    for (uint32_t nb = 1; nb <= 2; ++nb)
        for (size_t n : ns)
            for (size_t count : counts)
                for (uint32_t max_blobs : {0u, 1u, 2u}) {
                    const uint32_t group = g2_batch_group(n, nb, count, max_blobs);
                    // batched = 0 exactly when the rule says so: a blob above one launch, or no group of two fits; a group of one runs all the same
                    const bool want_batched = n <= G2MSM_MAX_LAUNCH && caps_hold(n, nb, 2);
                    G2_INVARIANT(g2_batch_shares(n, nb) == want_batched && group >= 1);
                    // the group: all three caps hold; one more blob would break one of them, or pass max_blobs, or the count
                    G2_INVARIANT(group <= count && (!max_blobs || group <= max_blobs) && caps_hold(n, nb, group));
                    const bool result_binds = !results_fit(n, nb, group + 1), entry_binds = !entries_fit(n, group + 1);
                    G2_INVARIANT(!caps_hold(n, nb, group + 1) || group == count || (max_blobs && group == max_blobs));
                    const G2Plan p = g2_make_plan(n, nb, group, WAVE_SLOTS);
                    failures += check_plan(p, n, nb, count, max_blobs, group);
                    if (out)
                        fprintf(out, "n=%zu nb=%u count=%zu max=%u batched=%d group=%u c=%d W=%d G=%u entries=%zu nl=%u seg=%u small=%d scan1=%d launches=%u bytes=%zu result_binds=%d entry_binds=%d\n",
                                n, nb, count, max_blobs, (int)want_batched, group, p.c, p.W, p.G, p.entries(), p.nl, p.seg, (int)p.sort.sort_small, (int)(p.G <= SCAN1_MAX),
                                p.launches, p.workspace_bytes, (int)result_binds, (int)entry_binds);
                }
    // the largest launch: no two blobs fit, the group is one blob and its plan passes
    for (uint32_t nb = 1; nb <= 2; ++nb) {
        const size_t n = G2MSM_MAX_LAUNCH, count = 4; const uint32_t max_blobs = 0;
        G2_INVARIANT(!g2_batch_shares(n, nb) && g2_batch_group(n, nb, count, max_blobs) == 1);
        failures += check_plan(g2_make_plan(n, nb, 1, WAVE_SLOTS), n, nb, count, max_blobs, 1);
    }
    // rejections
    {
        const size_t n = 16, count = 0; const uint32_t nb = 1, max_blobs = 0;
        const char* error = nullptr;
        G2_INVARIANT(g2_batch_group((size_t)G2MSM_MAX_LAUNCH + 1, 1, 64, 0) == 0 && !g2_batch_shares((size_t)G2MSM_MAX_LAUNCH + 1, 1));      // above one launch: parts
        G2_INVARIANT(g2_batch_group(0, 1, 64, 0) == 0 && g2_batch_group(16, 3, 64, 0) == 0 && g2_batch_group(16, 0, 64, 0) == 0);
        G2_INVARIANT(g2_plan_status(g2_make_plan(0, 1, 1, WAVE_SLOTS), 0, G2_RESULT_CAP, &error) == KZG_ERR_INVALID_ARG);
        G2_INVARIANT(g2_plan_status(g2_make_plan(0, 1, 2, WAVE_SLOTS), 0, G2_RESULT_CAP, &error) == KZG_ERR_INVALID_ARG);
        G2_INVARIANT(g2_plan_status(g2_make_plan(16, 3, 1, WAVE_SLOTS), 16, G2_RESULT_CAP, &error) == KZG_ERR_INVALID_ARG);
        G2_INVARIANT(g2_plan_status(g2_make_plan(16, 3, 2, WAVE_SLOTS), 16, G2_RESULT_CAP, &error) == KZG_ERR_INVALID_ARG);
        G2_INVARIANT(g2_plan_status(g2_make_plan(16, 1, 0, WAVE_SLOTS), 16, G2_RESULT_CAP, &error) == KZG_ERR_INVALID_ARG);
        G2_INVARIANT(g2_plan_status(g2_make_plan((size_t)G2MSM_MAX_LAUNCH + 1, 1, 1, WAVE_SLOTS), (size_t)G2MSM_MAX_LAUNCH + 1, G2_RESULT_CAP, &error) == KZG_ERR_INVALID_ARG && error);
        G2_INVARIANT(g2_plan_status(g2_make_plan(G2MSM_MAX_LAUNCH, 2, 1, WAVE_SLOTS), G2MSM_MAX_LAUNCH, G2_RESULT_CAP, &error) == KZG_OK);
        G2_INVARIANT(g2_plan_status(g2_make_plan(16, 2, 1, WAVE_SLOTS), 16, 100, &error) == KZG_ERR_INVALID_ARG && error);       // 128 result points
        G2_INVARIANT(g2_plan_status(g2_make_plan(4096, 2, 96, WAVE_SLOTS), 4096, G2_RESULT_CAP, &error) == KZG_ERR_INVALID_ARG && error);    // 8 256 result values
        G2_INVARIANT(g2_plan_status(g2_make_plan((size_t)1 << 20, 1, 7, WAVE_SLOTS), (size_t)1 << 20, G2_RESULT_CAP, &error) == KZG_ERR_INVALID_ARG && error);   // 19 x 7 x 2^20 entries
        G2_INVARIANT(g2_plan_status(g2_make_plan(4096, 2, 95, WAVE_SLOTS), 4096, G2_RESULT_CAP, &error) == KZG_OK);
    }
    return failures;
}
}  // namespace g2grid
