// tests/hostcheck/g2msm_plan_grid.h — the cases and invariants of the G2 MSM planner (csrc/g2msm_plan.h), shared by g2msm_plancheck.cpp and
// the sanitizer program g2_sanitize_main.cpp: every n in 1 .. 2^20 that is a power of two or one beside it, and every n at which the plan
// changes shape (window bits, sort form, scan form, saturated lanes) with its two neighbours.
#pragma once
#include <cstdio>
#include <set>
#include <vector>

#include "g2msm_plan.h"

namespace g2grid {
using namespace kzg;

constexpr uint32_t WAVE_SLOTS = 256 * 4 * G2_ACC_WAVES;        // a 256-CU device

// the fields that make a plan's SHAPE: which kernels run and how the buffers are indexed, not how large they are
inline bool same_shape(const G2Plan& a, const G2Plan& b) {
    return a.c == b.c && a.W == b.W && a.B == b.B && a.T == b.T && a.m == b.m && a.sort.sort_small == b.sort.sort_small &&
           (a.G <= SCAN1_MAX) == (b.G <= SCAN1_MAX) && (a.nl == WAVE_SLOTS * 64) == (b.nl == WAVE_SLOTS * 64) && a.launches == b.launches;
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
            if (b - a <= 1 || same_shape(g2_make_plan(a, 1, WAVE_SLOTS), g2_make_plan(b, 1, WAVE_SLOTS))) {
                if (b - a == 1 && !same_shape(g2_make_plan(a, 1, WAVE_SLOTS), g2_make_plan(b, 1, WAVE_SLOTS))) { ns.insert(a); ns.insert(b); }
                continue;
            }
            const size_t mid = a + (b - a) / 2;
            todo.push_back({a, mid});
            todo.push_back({mid, b});
        }
    }
    return std::vector<size_t>(ns.begin(), ns.end());
}

#define G2_INVARIANT(c) do { if (!(c)) { ++failures; fprintf(stderr, "g2msm_plancheck: n=%zu nb=%u: %s\n", n, nb, #c); } } while (0)

// prints one line per plan to `out` (may be null); returns the number of violated invariants
inline int run(FILE* out) {
    int failures = 0;
    const std::vector<size_t> ns = cases();
    const size_t point = 72 * 4;
    for (uint32_t nb = 1; nb <= 2; ++nb) {
        G2Plan prev{};
        bool have_prev = false;
        for (size_t n : ns) {
            const G2Plan p = g2_make_plan(n, nb, WAVE_SLOTS);
            const char* error = nullptr;
            const int32_t st = g2_plan_status(p, n, MSM_MAX_OUT * 32 / G2_WIRE_WORDS, &error);
            G2_INVARIANT(st == KZG_OK && error == nullptr);                       // every n of the grid passes its own status function
            G2_INVARIANT(p.c == generic_window(n, 1) && p.W == (255 + p.c - 1) / p.c && p.B == (1u << (p.c - 1)) && p.G == (uint32_t)p.W * p.B);
            G2_INVARIANT(p.nl % 256 == 0 && p.nl >= 256 && p.nl <= WAVE_SLOTS * 64);
            // entries per lane: the equal share, whatever the scalars -- never more than G2_SEG_MIN while the chip is not full, the share
            // of a full chip rounded up after that
            G2_INVARIANT((size_t)p.seg * p.nl >= p.entries() && (size_t)(p.seg - 1) * p.nl < p.entries());
            G2_INVARIANT(p.seg <= std::max<size_t>(G2_SEG_MIN, (p.entries() + (size_t)WAVE_SLOTS * 64 - 1) / ((size_t)WAVE_SLOTS * 64)));
            G2_INVARIANT(p.fin_adds_bound() <= WAVE_SLOTS + 7);                   // bucket kernel: the partials of one bucket over the 64 lanes of a wave
            G2_INVARIANT(p.T * p.m == p.B && p.T >= 2 && p.T <= G2_RED_T && (p.T & (p.T - 1)) == 0);
            G2_INVARIANT(p.n_out == (uint32_t)p.W * nb && p.n_out * G2_WIRE_WORDS <= MSM_MAX_OUT * 32);
            // the workspace is as large as the kernels index it (g2msm.hip launch arguments)
            G2_INVARIANT(p.bytes[G2WS_HEAD] >= (size_t)p.G * point && p.bytes[G2WS_BUCKET] >= (size_t)p.G * point && p.bytes[G2WS_CONT] >= (size_t)p.nl * point);
            G2_INVARIANT(p.bytes[G2WS_CHUNK_S] >= (size_t)p.n_chunks() * point && p.bytes[G2WS_CHUNK_TMP] >= (size_t)p.n_chunks() * point &&
                         p.bytes[G2WS_CHUNK_A] >= (size_t)p.n_chunks() * point);
            G2_INVARIANT(p.sort.bytes[WS_SORTED] >= p.entries() * 4 && p.sort.bytes[WS_DIGITS] >= p.entries() * 4);
            G2_INVARIANT(p.sort.bytes[WS_COUNT] >= (size_t)p.G * 4 && p.sort.bytes[WS_OFFS] >= ((size_t)p.G + 1) * 4);
            G2_INVARIANT(!p.sort.tables && !p.sort.sort2 && !p.sort.lean_sort && p.sort.batch == 1 && p.sort.n == p.n);
            G2_INVARIANT(p.entries() < ((size_t)1 << 31));                        // 32-bit positions, the sign bit of an entry free
            if (have_prev && same_shape(prev, p)) G2_INVARIANT(p.workspace_bytes >= prev.workspace_bytes);      // monotone within a shape
            if (out)
                fprintf(out, "n=%zu nb=%u c=%d W=%d B=%u nl=%u seg=%u T=%u m=%u small=%d scan1=%d launches=%u n_out=%u bytes=%zu\n", n, nb, p.c, p.W, p.B, p.nl,
                        p.seg, p.T, p.m, (int)p.sort.sort_small, (int)(p.G <= SCAN1_MAX), p.launches, p.n_out, p.workspace_bytes);
            prev = p;
            have_prev = true;
        }
    }
    // rejections
    {
        const size_t n = 0; const uint32_t nb = 1;
        const char* error = nullptr;
        G2_INVARIANT(g2_plan_status(g2_make_plan(0, 1, WAVE_SLOTS), 0, 8192, &error) == KZG_ERR_INVALID_ARG);
        G2_INVARIANT(g2_plan_status(g2_make_plan(16, 3, WAVE_SLOTS), 16, 8192, &error) == KZG_ERR_INVALID_ARG);
        G2_INVARIANT(g2_plan_status(g2_make_plan((size_t)G2MSM_MAX_LAUNCH + 1, 1, WAVE_SLOTS), (size_t)G2MSM_MAX_LAUNCH + 1, 8192, &error) == KZG_ERR_INVALID_ARG && error);
        G2_INVARIANT(g2_plan_status(g2_make_plan(G2MSM_MAX_LAUNCH, 2, WAVE_SLOTS), G2MSM_MAX_LAUNCH, 8192, &error) == KZG_OK);
        G2_INVARIANT(g2_plan_status(g2_make_plan(16, 2, WAVE_SLOTS), 16, 100, &error) == KZG_ERR_INVALID_ARG && error);       // 128 result points
    }
    return failures;
}
}  // namespace g2grid
