// ntt_plan.h — the pass policy of the Fr NTT driver (ntt.hip ntt_run): from log n, the direction, the CU count and the tile override to everything
// the driver decides before its first launch -- the split into passes, the arguments each pass's kernel receives, the ping-pong buffers, the grids,
// the per-element twiddle arrays to fetch, the one kernel instantiation of the transform and the workspace bytes.  Pure host code: no HIP type, no
// kzg_ctx, no allocation; also compiled with g++ by tests/hostcheck/ntt_plancheck.cpp, which pins every plan of a fixed grid
// (tests/golden/ntt_plans.txt).  The comments that quote measurements are the record of why a threshold has its value.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "host_log2.h"

namespace kzg {

constexpr int NTT_MAX_LOG = 28;                    // the largest domain: Fr has 2^28-th roots of unity
constexpr int NTT_KMAX = 10;                       // radix bits of one pass: P = ceil(log n / 10) passes
constexpr int NTT_MAX_PASSES = (NTT_MAX_LOG + NTT_KMAX - 1) / NTT_KMAX;
constexpr int NTT_EPT = 4;                         // elements per thread in the load / store phases = one radix-4 butterfly per thread and step
// Two tile sizes (round 4).  2 048 elements / 512 threads, one workgroup per CU: transforms of >= 2^19 elements (>= 256 tiles per pass).
// 1 024 elements / 256 threads, two workgroups per CU: smaller transforms -- twice the workgroups (2^18: 256 instead of 128 on 256
// CUs; one tile of a <= 1 024-point transform in half the threads) and two independent barrier domains per CU:
// 2^12 / 2^16 / 2^18 0.052 / 0.062 / 0.073 -> 0.040 / 0.046 / 0.057 ms per call; at 2^20 the big tile stays ahead (0.140 against 0.147).
constexpr int NTT_TILE_LOG_BIG = 11, NTT_TILE_LOG_SMALL = 10;
// measured per call, small / big tile (tools/archive/time_ntt_variants.py, KZG_NTT_TILE_LOG=10 / 11): 2^10 0.034 / 0.043, 2^14 0.045 / 0.058,
// 2^17 0.055 / 0.067, 2^18 0.059 / 0.071, 2^19 0.086 / 0.082, 2^20 0.155 / 0.136, 2^21 0.280 / 0.297, 2^22 0.537 / 0.562, 2^23 1.195 /
// 1.246, 2^24 2.46 / 2.52, 2^25 5.31 / 5.34, 2^26 12.1 / 11.1 ms
// round 6: 2^25 moved to the small tile (its passes are 9 + 8 + 8 bits: the slim instantiation below, three workgroups per CU: 5.24 -> 4.95 ms; 2^26 stays: 10.9 against 11.5)
inline bool ntt_small_tile_pays(int log_n) { return log_n <= 18 || (log_n >= 21 && log_n <= 25); }
constexpr int NTT_LO_BITS = 10;                    // the two-level twiddle table: w^t for t < 2^min(log n, 10), and w^(t 2^10)
// HBM capacity spent to remove work (like the MSM window tables): the inter-pass twiddle of every element as one 32-byte word,
// 32 MiB per pass boundary at 2^20; kept per (device, log n, direction, boundary) for transforms of up to 2^22 elements.
constexpr int NTT_FULL_TW_MAX_LOG = 22;

struct NttPassArgs {
    int log_n, K, log_s;          // this pass
    int next_K, next_log_s;       // the pass after it (next_K = 0: this is the last pass)
    int scale_log_n;              // last pass: >= 0 multiplies by (2^scale_log_n)^-1; -1: no factor left (forward transform, or the inverse's 1 / n
                                  // folded into the twiddle array of the previous pass boundary): the outputs are only reduced (fe_reduce_small)
    uint32_t n_tiles;
};

enum NttKernel {                  // the instantiations of k_ntt_pass<TILE_LOG, KMAX_T>; one per transform
    NTT_K_BIG,                    // <11, 10>: 512 threads, one workgroup per CU
    NTT_K_SMALL,                  // <10, 10>: 256 threads, two per CU
    NTT_K_SLIM7, NTT_K_SLIM8, NTT_K_SLIM9,   // <10, 7 / 8 / 9>: 256 threads, three per CU
    NTT_KERNELS
};
enum NttBuf { NTT_BUF_CALLER, NTT_BUF_DATA, NTT_BUF_TMP };      // the caller's data, ws.data, ws.tmp

struct NttPass {
    NttPassArgs args;             // the very struct the kernel receives
    int src, dst;                 // NttBuf
    uint32_t grid;
    bool tw;                      // a per-element twiddle array is wanted for the boundary after this pass ...
    bool tw_scaled;               // ... and it carries the inverse transform's 1 / n
};
struct NttPlan {
    int log_n;
    bool inverse;
    int n_passes;
    NttPass pass[NTT_MAX_PASSES];
    int kernel, threads;          // NttKernel and its workgroup size
    size_t bytes_data, bytes_tmp; // to reserve in ws.data / ws.tmp (0: not used)
};

// cus: CUs of the device; tile_env: KZG_NTT_TILE_LOG = 10 / 11: one tile size at every transform size (tests cover both kernels everywhere), else by size.
// 1 <= log_n <= NTT_MAX_LOG.
inline NttPlan ntt_plan(int log_n, bool inverse, int cus, int tile_env) {
    NttPlan p{};
    p.log_n = log_n;
    p.inverse = inverse;
    const size_t n = (size_t)1 << log_n;
    // (2^20 as THREE passes of 7 + 7 + 6 bits on slim workgroups: 0.1305 / 0.1322 ms against 0.1333 for 10 + 10 -- 1.5 % for 60 % more HBM traffic: not taken;
    //  2^15 .. 2^19 lose 2 .. 13 % that way)
    const int P = (log_n + NTT_KMAX - 1) / NTT_KMAX;
    p.n_passes = P;
    int Ks[NTT_MAX_PASSES + 1] = {}, kmax = 0;          // (one past the end: the "next pass" of the last one)
    for (int pi = 0; pi < P; ++pi) { Ks[pi] = log_n / P + (pi < log_n % P ? 1 : 0); kmax = std::max(kmax, Ks[pi]); }
    // Round 6: the radix bits of the widest pass decide the per-workgroup twiddle table.  With K <= 9 a 1 024-element workgroup needs 41.5 / 43.8 / 48.4 KB of LDS
    // instead of 57.6, THREE fit a CU and at 145 VGPRs run three waves per SIMD -- the instantiations k_ntt_pass<10, 7 / 8 / 9>; fill and drain of one tile then
    // overlap the butterfly stages of two others.  Same-box A/B against the KMAX = 10 instantiation (two per CU, early twiddle read), ms per transform
    // (tools/time_ntt.py): 2^8 0.0267 -> 0.0254, 2^12 0.0385 -> 0.0372, 2^16 0.0450 -> 0.0430, 2^18 0.0552 -> 0.0531, 2^21 0.2723 -> 0.2423, 2^22 0.5213 -> 0.4880,
    // 2^23 1.168 -> 1.082, 2^24 2.430 -> 2.268, 2^25 5.24 (2 048-element tile) -> 4.95.  2^10, 2^19, 2^20 and 2^26 .. 2^30 have a 10-bit pass and stay as they were.
    const bool small_tile = tile_env == NTT_TILE_LOG_SMALL || (tile_env != NTT_TILE_LOG_BIG && ntt_small_tile_pays(log_n));
    const int slim = small_tile && kmax <= 9 ? std::max(kmax, 7) : 0;
    const int tile_log = small_tile ? NTT_TILE_LOG_SMALL : NTT_TILE_LOG_BIG;
    p.kernel = slim ? NTT_K_SLIM7 + (slim - 7) : small_tile ? NTT_K_SMALL : NTT_K_BIG;
    p.threads = (1 << tile_log) / NTT_EPT;
    // big tile: one workgroup per CU (97 KB of LDS); small tile: two (58 KB each); a workgroup walks its tiles with the next one's words prefetched
    const uint32_t per_cu = slim ? 3u : small_tile ? 2u : 1u;
    // buffers: data -> A -> (B ->) data; a single pass works in place (one tile holds the whole transform)
    p.bytes_data = P > 1 ? n * 32 : 0;
    p.bytes_tmp = P > 2 ? n * 32 : 0;
    int log_ncur = 0;
    for (int pi = 0; pi < P; ++pi) {
        NttPass& s = p.pass[pi];
        NttPassArgs& a = s.args;
        const bool last = pi == P - 1;
        a.log_n = log_n;
        a.K = Ks[pi];
        log_ncur += a.K;
        a.log_s = log_n - log_ncur;
        a.next_K = last ? 0 : Ks[pi + 1];
        a.next_log_s = last ? 0 : log_n - (log_ncur + Ks[pi + 1]);
        const uint32_t n_units = (uint32_t)(n >> a.K);
        const uint32_t C = 1u << (tile_log - a.K);
        a.n_tiles = (n_units + C - 1) / C;
        s.src = pi == 0 ? NTT_BUF_CALLER : NTT_BUF_DATA + ((pi - 1) & 1);
        s.dst = last ? NTT_BUF_CALLER : NTT_BUF_DATA + (pi & 1);
        s.grid = std::min<uint32_t>(a.n_tiles, (uint32_t)cus * per_cu);
        s.tw = !last && log_n <= NTT_FULL_TW_MAX_LOG;
        s.tw_scaled = s.tw && inverse && pi == P - 2;       // the boundary in front of the last pass carries the scaling
        // the last pass of an inverse transform scales unless that array did: the plan says "fold wanted" (ntt_plan_fold_missing is the other half)
        a.scale_log_n = last && inverse && !(pi > 0 && p.pass[pi - 1].tw_scaled) ? log_n : -1;
    }
    return p;
}
// The one thing decided at run time: the array that was to carry the 1 / n could not be allocated, the kernel in front of the last pass looks its
// twiddles up itself, so the last pass scales after all.  The driver calls this when the fetch of a tw_scaled array returned none.
inline void ntt_plan_fold_missing(NttPlan& p) { p.pass[p.n_passes - 1].args.scale_log_n = p.log_n; }

}  // namespace kzg
