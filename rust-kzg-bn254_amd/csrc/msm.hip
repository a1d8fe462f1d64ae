// msm.hip — host orchestration of the G1 MSM kernels (msm_kernels.h).
// Replaces `G1Projective::msm(..)` + `.into_affine()` at prover/src/kzg.rs:100-101, :121-122 and
// primitives/src/helpers.rs:332-336.
//
// Two modes share the digit / sort / accumulate kernels:
//   table mode   (SRS with precomputed window tables T_w[i] = 2^(c w) P_i, built once at upload — HBM capacity is
//                 spent to remove work): every (scalar, window) entry adds +-T_w[i] into ONE set of 2^(c-1) buckets;
//                 W n mixed adds, one shuffle-based bucket reduction, no Horner.
//   generic mode (caller-provided bases, e.g. g1_lincomb; tiny or huge SRS): W bucket sets, per-window reduction,
//                 Horner over the W window sums on the host.
// What a launch does is decided in msm_plan.h (make_plan, msm_plan_status) before anything is enqueued; what the host does with its result
// points is host_msm_epilogue.h.  This file reserves, launches and waits.
#include "engine.h"
#include <new>
#include "msm_kernels.h"
#include "host_msm_epilogue.h"
#include "host_pairing.h"      // fr_wire_to_canonical (KZG_DEBUG_SORT)

#include <algorithm>
#include <cstdlib>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

namespace kzg {

void MsmWorkspace::release() {
    DeviceBuffer* all[] = {&scalars, &bases, &bases_wire, &digits, &sorted, &count, &blockbase, &sort_tmp, &sort_key, &sort_small, &offs, &block_sums,
                           &head, &cont, &blob, &bucket, &chunkS, &chunkTmp, &chunkA, &out_wire};
    for (auto* b : all) b->release();
    if (pinned_out) { (void)hipHostFree(pinned_out); pinned_out = nullptr; }
    if (ev_ready) { for (auto& e : ev) (void)hipEventDestroy(e); ev_ready = false; }
    if (ev_done) { (void)hipEventDestroy(ev_done); ev_done = nullptr; }
    if (ev_sorted) { (void)hipEventDestroy(ev_sorted); ev_sorted = nullptr; }
}

// What msm_enqueue leaves in flight on its stream; msm_finish waits for it and runs the host epilogue.
struct Pending {
    Plan p;
    uint32_t out_off = 0;    // first point of this launch's results in the pinned result buffer
    bool profiled = true;    // the workspace's phase events belong to this launch (the last one enqueued)
};
struct MsmPending {
    Pending part[MSM_MAX_PARTS];
    uint32_t n_parts = 0;
};

// f(std::integral_constant<T, V>{}) for the V among Vs that equals v: a run-time value picks a template argument and the launch is written once
template <auto... Vs, class T, class F>
static void dispatch(T v, F&& f) { (void)(((v == Vs) && (f(std::integral_constant<T, Vs>{}), true)) || ...); }

// one launch on its way to the stream: what every enqueue_* below reads
struct Launch {
    kzg_ctx* ctx;
    MsmWorkspace& ws;
    hipStream_t st;
    const MsmBases& bases;
    const uint4* d_scalars;
    const Plan& p;
    uint32_t* d_out;         // this launch's window of the pinned result buffer, as the device sees it
    bool prof;
};
#define KZG_MARK(i) do { if (L.prof) KZG_HIP_TRY(L.ctx, hipEventRecord(L.ws.ev[i], L.st)); } while (0)

static int32_t set_sort_lds_attributes(kzg_ctx* ctx) {
    if (ctx->lds_attr_set) return KZG_OK;
    KZG_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_sort_hist), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SORT1_MAX_LDS));
    KZG_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_sort_scatter), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SORT1_MAX_LDS));
    KZG_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_sort2_scatter1_lds<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)((3 * SORT2_MAX_BINS + SORT2_P1_THREADS * 31) * 4)));
    KZG_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_sort2_scatter1_lds<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)((3 * SORT2_MAX_BINS + SORT2_P1_THREADS * 31) * 4 + SORT2_P1_THREADS * 31 * 2)));
    KZG_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_sort2_scatter1_lds<true, 32>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)((3 * SORT2_MAX_BINS + SORT2_P1_THREADS * 32) * 4 + SORT2_P1_THREADS * 32 * 2)));
    ctx->lds_attr_set = true;
    return KZG_OK;
}

static void scan_counts(const Launch& L) {
    const Plan& p = L.p;
    MsmWorkspace& ws = L.ws;
    if (p.G <= SCAN1_MAX) {
        hipLaunchKernelGGL(k_scan_counts_1wg<false>, dim3(1), dim3(SCAN1_THREADS), 0, L.st, ws.count.as<uint32_t>(), p.G, ws.offs.as<uint32_t>(), (uint32_t*)nullptr);
    } else {
        const uint32_t nb = p.scan_blocks();
        hipLaunchKernelGGL(k_scan_block_sums, dim3(nb), dim3(SCAN_THREADS), 0, L.st, ws.count.as<uint32_t>(), p.G, ws.block_sums.as<uint32_t>());
        hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(SCAN_THREADS), 0, L.st, ws.block_sums.as<uint32_t>(), nb);
        hipLaunchKernelGGL(k_scan_final, dim3(nb), dim3(SCAN_THREADS), 0, L.st, ws.count.as<uint32_t>(), p.G, ws.block_sums.as<uint32_t>(), ws.offs.as<uint32_t>());
    }
}

// two-level sort straight from the scalars (no digit array)
static int32_t sort_two_level(const Launch& L, const PolyPtrs* poly_ptrs) {
    const Plan& p = L.p;
    MsmWorkspace& ws = L.ws;
    hipStream_t st = L.st;
    uint32_t* small = ws.sort_small.as<uint32_t>();
    uint32_t* ccount = small;                       // Hb
    uint32_t* cstart = small + (p.Hb + 1);          // Hb + 1
    uint32_t* tstart = small + 2 * (p.Hb + 1);      // Hb + 1
    uint32_t* tile_bin = small + 3 * (p.Hb + 1);    // tiles2cap
    uint32_t* bin_cap = tile_bin + p.tiles2cap;     // 1: the LARGE-bin threshold of this launch (k_sort2_scan)
    uint32_t* blockbase = ws.blockbase.as<uint32_t>();
    uint32_t* tmp1 = ws.sort_tmp.as<uint32_t>();
    KZG_HIP_TRY(L.ctx, hipMemsetAsync(ccount, 0, (size_t)p.Hb * 4, st));
    uint8_t* tmpk = p.naf ? ws.sort_key.as<uint8_t>() : nullptr;
    const uint32_t poly_len = p.polys ? p.n / p.polys : 0u;
    PolyPtrs ptrs{};
    if (poly_ptrs) ptrs = *poly_ptrs;
    if (p.naf)
        dispatch<32, NAF_DIGITS>(p.ND, [&](auto nd) {
            constexpr int ND = decltype(nd)::value;
            hipLaunchKernelGGL(k_naf_digits<ND>, dim3(p.tiles1), dim3(256), ((size_t)p.Hb + (11 + ND) * 256) * 4, st, L.d_scalars, p.n, p.c, p.tile1, p.Hb, ccount,
                               blockbase, ws.digits.as<uint4>(), poly_len, ptrs);
        });
    else
        hipLaunchKernelGGL(k_sort2_scalars<false>, dim3(p.tiles1), dim3(256), (size_t)p.Hb * 4, st, L.d_scalars, p.n, p.c, p.W, p.tile1, p.Hb, ccount,
                           blockbase, (const uint32_t*)nullptr, p.idx_stride, (uint32_t*)nullptr);
    KZG_MARK(1);
    hipLaunchKernelGGL(k_sort2_scan, dim3(1), dim3(512), 0, st, ccount, p.Hb, cstart, tstart, tile_bin, ws.count.as<uint32_t>(), bin_cap);
    if (p.naf) {
        const size_t lds1 = ((size_t)3 * p.Hb + (size_t)SORT2_P1_THREADS * p.W) * 4 + (size_t)SORT2_P1_THREADS * p.W * 2;
        dispatch<32, NAF_DIGITS>(p.ND, [&](auto nd) {
            hipLaunchKernelGGL((k_sort2_scatter1_lds<true, decltype(nd)::value>), dim3(p.tiles1), dim3(SORT2_P1_THREADS), lds1, st, ws.digits.as<uint4>(), p.n, p.c, p.W,
                               p.tile1, p.Hb, blockbase, (const uint32_t*)cstart, p.idx_stride, tmp1, tmpk, poly_len);
        });
    } else if (p.W > 31) {                              // (more windows than the LDS staging holds: pass 1 scatters directly)
        hipLaunchKernelGGL(k_sort2_scalars<true>, dim3(p.tiles1), dim3(256), (size_t)p.Hb * 4, st, L.d_scalars, p.n, p.c, p.W, p.tile1, p.Hb, ccount,
                           blockbase, (const uint32_t*)cstart, p.idx_stride, tmp1);
    } else {
        const size_t lds1 = ((size_t)3 * p.Hb + (size_t)SORT2_P1_THREADS * p.W) * 4;
        hipLaunchKernelGGL(k_sort2_scatter1_lds<false>, dim3(p.tiles1), dim3(SORT2_P1_THREADS), lds1, st, L.d_scalars, p.n, p.c, p.W, p.tile1, p.Hb,
                           blockbase, (const uint32_t*)cstart, p.idx_stride, tmp1, (uint8_t*)nullptr);
    }
    KZG_MARK(2);
    dispatch<true, false>(p.naf, [&](auto naf) {
        constexpr bool NAF = decltype(naf)::value;
        hipLaunchKernelGGL(k_sort2_hist2<NAF>, dim3(p.tiles2cap), dim3(256), 0, st, tmp1, cstart, tstart, tile_bin, p.Hb, ws.count.as<uint32_t>(), blockbase,
                           (const uint8_t*)tmpk);
        hipLaunchKernelGGL(k_sort2_bin<NAF>, dim3(p.Hb), dim3(SORT2_BIN_THREADS), 0, st, tmp1, cstart, p.Hb, ws.count.as<uint32_t>(), ws.offs.as<uint32_t>(),
                           ws.sorted.as<uint32_t>(), (const uint32_t*)bin_cap, (const uint8_t*)tmpk);
        hipLaunchKernelGGL(k_sort2_scatter2<NAF>, dim3(p.tiles2cap), dim3(256), 0, st, tmp1, cstart, tstart, tile_bin, p.Hb, ws.offs.as<uint32_t>(), blockbase,
                           ws.sorted.as<uint32_t>(), (const uint8_t*)tmpk);
    });
    KZG_MARK(3);
    return KZG_OK;
}

// small table-mode MSM (one bucket set): digits + histogram in one pass, the scan leaves the scatter's cursors and clears the counters
// it read -- three launches instead of four launches and two memsets (each ~3-5 us of a ~100 us commitment)
static int32_t sort_lean(const Launch& L, uint32_t clean_g) {
    const Plan& p = L.p;
    MsmWorkspace& ws = L.ws;
    const uint32_t entries = (uint32_t)p.entries(), ge = (uint32_t)((p.entries() + 255) / 256);
    if (clean_g < p.G) KZG_HIP_TRY(L.ctx, hipMemsetAsync(ws.count.p, 0, (size_t)p.G * 4, L.st));
    hipLaunchKernelGGL(k_msm_digits, dim3((p.n + 255) / 256), dim3(256), 0, L.st, L.d_scalars, p.n, p.n, p.c, p.W, ws.digits.as<uint32_t>(), ws.count.as<uint32_t>());
    KZG_MARK(1);
    hipLaunchKernelGGL(k_scan_counts_1wg<true>, dim3(1), dim3(SCAN1_THREADS), 0, L.st, ws.count.as<uint32_t>(), p.G, ws.offs.as<uint32_t>(), ws.blockbase.as<uint32_t>());
    KZG_MARK(2);
    hipLaunchKernelGGL(k_sort_small_scatter, dim3(ge), dim3(256), 0, L.st, ws.digits.as<uint32_t>(), entries, p.n, p.set_len, p.B,
                       ws.offs.as<uint32_t>(), ws.blockbase.as<uint32_t>(), p.idx_stride, (uint32_t)p.W, ws.sorted.as<uint32_t>(), 1);
    KZG_MARK(3);
    ws.count_zero_ptr = ws.count.p;
    ws.count_zero_g = p.G;
    return KZG_OK;
}

// digit array, then the global-atomic sort (few entries) or the single-pass tiled sort
static int32_t sort_from_digits(const Launch& L) {
    const Plan& p = L.p;
    MsmWorkspace& ws = L.ws;
    hipStream_t st = L.st;
    const uint32_t n_total = p.n * p.batch;
    // the scatters add (set / windows_per_msm) * n to an entry's index (batched MSMs over concatenated bases): no set reaches this divisor,
    // so over shared bases the term is 0
    const uint32_t windows_per_msm = p.shared_bases ? 0xFFFFFFFFu : (uint32_t)p.W;
    KZG_HIP_TRY(L.ctx, hipMemsetAsync(ws.count.p, 0, (size_t)p.G * 4, st));
    hipLaunchKernelGGL(k_msm_digits, dim3((n_total + 255) / 256), dim3(256), 0, st, L.d_scalars, n_total, p.n, p.c, p.W, ws.digits.as<uint32_t>(), (uint32_t*)nullptr);
    KZG_MARK(1);
    if (p.sort_small) {
        const uint32_t entries = (uint32_t)p.entries(), ge = (uint32_t)((p.entries() + 255) / 256);
        KZG_HIP_TRY(L.ctx, hipMemsetAsync(ws.blockbase.p, 0, (size_t)p.G * 4, st));
        hipLaunchKernelGGL(k_sort_small_hist, dim3(ge), dim3(256), 0, st, ws.digits.as<uint32_t>(), entries, p.set_len, p.B, ws.count.as<uint32_t>());
        scan_counts(L);
        KZG_MARK(2);
        hipLaunchKernelGGL(k_sort_small_scatter, dim3(ge), dim3(256), 0, st, ws.digits.as<uint32_t>(), entries, p.n, p.set_len, p.B,
                           ws.offs.as<uint32_t>(), ws.blockbase.as<uint32_t>(), p.idx_stride, windows_per_msm, ws.sorted.as<uint32_t>());
    } else {
        const size_t lds_bytes = (size_t)p.B * 4;
        hipLaunchKernelGGL(k_sort_hist, dim3(p.tiles), dim3(256), lds_bytes, st, ws.digits.as<uint32_t>(), p.set_len, p.tile_len,
                           p.tiles_per_set, p.B, ws.count.as<uint32_t>(), ws.blockbase.as<uint32_t>());
        scan_counts(L);
        KZG_MARK(2);
        hipLaunchKernelGGL(k_sort_scatter, dim3(p.tiles), dim3(256), lds_bytes, st, ws.digits.as<uint32_t>(), p.n, p.set_len, p.tile_len,
                           p.tiles_per_set, p.B, ws.offs.as<uint32_t>(), ws.blockbase.as<uint32_t>(), p.idx_stride,
                           windows_per_msm, ws.sorted.as<uint32_t>());
    }
    KZG_MARK(3);
    return KZG_OK;
}

// scalars -> entries sorted by bucket (ws.sorted) and the buckets' offsets (ws.offs); profiling events 0 .. 4
static int32_t enqueue_sort(const Launch& L, const PolyPtrs* poly_ptrs) {
    const Plan& p = L.p;
    kzg_ctx* ctx = L.ctx;
    MsmWorkspace& ws = L.ws;
    if (p.bitsum) {                                         // (bit sums read the scalars themselves: the phases are empty)
        for (int i = 0; i <= 4; ++i) KZG_MARK(i);
        return KZG_OK;
    }
    { int32_t rc = set_sort_lds_attributes(ctx); if (rc != KZG_OK) return rc; }
    // Staggered start.  Two MSMs enqueued back to back on two streams (the fill of a pipeline) run their phases in lock-step: both sort
    // (memory-bound) and then both accumulate (VALU-bound), instead of one sorting beside the other's accumulate as in steady state,
    // where MSM k + 2 is only enqueued once MSM k is done.  So this launch starts behind the SORT of the previous launch of the context
    // when that went to another stream -- a no-op in steady state (that sort finished long ago), the natural stagger at the fill:
    // 20-step regions (profiles/r04_ab_msm_stagger.txt): 2^17-pair steps, four per launch, 0.188 -> 0.183 ms per step; 2^18 / 2^19, two per launch,
    // -0.7 %; long regions unchanged.  Only GROUPED launches wait (the sharded streams): a single 2^20-pair MSM planned alone lost 0.7 %
    // (1.115 -> 1.122: its successor's sort starts 0.2 ms later and the first MSM runs on three wave slots either way).
    const bool stagger = p.tables && p.polys >= 2;
    if (stagger && ctx->last_sorted && ctx->last_sorted_stream != L.st) KZG_HIP_TRY(ctx, hipStreamWaitEvent(L.st, ctx->last_sorted, 0));
    KZG_MARK(0);
    // what an earlier small sort left of `count` (see k_scan_counts_1wg<true>); every other path writes the counters as it likes
    const uint32_t clean_g = ws.count_zero_ptr == ws.count.p ? ws.count_zero_g : 0;
    ws.count_zero_g = 0;
    const int32_t rc = p.sort2 ? sort_two_level(L, poly_ptrs) : p.lean_sort ? sort_lean(L, clean_g) : sort_from_digits(L);
    if (rc != KZG_OK) return rc;
    KZG_MARK(4);
    if (p.tables) {                                         // (recorded by every table-mode launch: the NEXT launch decides whether it waits)
        if (!ws.ev_sorted) KZG_HIP_TRY(ctx, hipEventCreateWithFlags(&ws.ev_sorted, hipEventDisableTiming));
        KZG_HIP_TRY(ctx, hipEventRecord(ws.ev_sorted, L.st));
        ctx->last_sorted = ws.ev_sorted;
        ctx->last_sorted_stream = L.st;
    }
    return KZG_OK;
}

// sorted entries -> partial sums per bucket head and per lane (ws.head, ws.cont); profiling event 5.  Nothing to do where the first
// reduction level reads the entries (fused) or the scalars (bit sums) itself.
static int32_t enqueue_accumulate(const Launch& L) {
    const Plan& p = L.p;
    MsmWorkspace& ws = L.ws;
    // (64- and 128-thread workgroups measured the same as 256; a set with an identity point, or caller bases: every entry is tested)
    if (!p.bitsum && !p.fused)
        dispatch<true, false>(!L.bases.identity_free, [&](auto identity_bases) {
            hipLaunchKernelGGL(k_msm_accumulate<decltype(identity_bases)::value>, dim3(p.nl / 256), dim3(256), 0, L.st, L.bases.points, ws.sorted.as<uint32_t>(),
                               ws.offs.as<uint32_t>(), p.G, ws.head.as<int32_t>(), (size_t)p.G, ws.cont.as<int32_t>(), (size_t)p.nl, p.idx_log, p.stride_adj);
        });
    KZG_MARK(5);
    return KZG_OK;
}

// tiny MSM: two launches (msm_kernels.h section 6e)
static int32_t reduce_bitsum(const Launch& L) {
    const Plan& p = L.p;
    dispatch<8, 16, 32>(p.bitsum_chunk, [&](auto chunk) {
        hipLaunchKernelGGL(k_bitsum_level1<decltype(chunk)::value>, dim3(p.bitsum_wg), dim3(256), 0, L.st, L.bases.points, L.bases.table_stride, L.d_scalars, p.n,
                           L.ws.chunkS.as<int32_t>());
    });
    KZG_MARK(6);
    hipLaunchKernelGGL(k_bitsum_level2, dim3(p.n_out), dim3(256), 0, L.st, L.ws.chunkS.as<int32_t>(), p.bitsum_wg, L.d_out);
    return KZG_OK;
}

// table mode: one sum per bit of the bucket index and the total, per group of 64 buckets and then per unit of 4 096
static int32_t reduce_tables(const Launch& L) {
    const Plan& p = L.p;
    MsmWorkspace& ws = L.ws;
    const uint32_t G1 = p.G1(), G1p = p.G1p();
    int32_t* x1 = ws.chunkS.as<int32_t>();
    dispatch<true, false>(p.quad1, [&](auto quads) {
        using LG = std::conditional_t<decltype(quads)::value, QuadLanes, PairLanes>;
        const uint32_t wgs = (G1 + LG::WG_GROUPS - 1) / LG::WG_GROUPS;          // WG_GROUPS groups of 64 buckets per workgroup
        if (p.fused)
            hipLaunchKernelGGL(k_msm_bucket_bits1_fused<LG>, dim3(wgs), dim3(LG::THREADS), 0, L.st, L.bases.points, ws.sorted.as<uint32_t>(), ws.offs.as<uint32_t>(), p.B,
                               p.idx_log, p.stride_adj, G1, x1, (size_t)7 * G1, L.d_out);
        else
            hipLaunchKernelGGL(k_msm_bucket_bits1<LG>, dim3(wgs), dim3(LG::THREADS), 0, L.st, ws.offs.as<uint32_t>(), p.B, p.nl, ws.head.as<int32_t>(), (size_t)p.G,
                               ws.cont.as<int32_t>(), (size_t)p.nl, G1, x1, (size_t)7 * G1, L.d_out);
    });
    KZG_MARK(6);
    if (p.polys && p.c == 7) {
        hipLaunchKernelGGL(k_batch_finish, dim3((p.polys + 63) / 64), dim3(64), 0, L.st, x1, (size_t)7 * G1, G1, L.d_out);
    } else if (G1 > 1) {                                    // (one group: its seven sums are the result points)
        const uint32_t waves2 = 7 * G1p;
        if (p.quad)
            hipLaunchKernelGGL(k_red_bits2q, dim3(waves2), dim3(256), 0, L.st, x1, (size_t)7 * G1, G1, G1p, L.d_out);
        else
            hipLaunchKernelGGL(k_red_bits2p, dim3((waves2 + 1) / 2), dim3(128), 0, L.st, x1, (size_t)7 * G1, G1, G1p, L.d_out);
    }
    return KZG_OK;
}

// generic mode: bucket sums, then per window sum_b (b + 1) V_b by chunks of m buckets
static int32_t reduce_generic(const Launch& L) {
    const Plan& p = L.p;
    MsmWorkspace& ws = L.ws;
    hipStream_t st = L.st;
    const uint32_t n_chunks = p.n_chunks(), n_windows = p.n_windows();
    const uint32_t gg = (p.G + 255) / 256;
    hipLaunchKernelGGL(k_msm_bucket_fin, dim3(gg), dim3(256), 0, st, ws.offs.as<uint32_t>(), p.G, p.nl, p.m, n_chunks, ws.head.as<int32_t>(), (size_t)p.G,
                       ws.cont.as<int32_t>(), (size_t)p.nl, ws.bucket.as<int32_t>(), (size_t)p.G);
    const uint32_t gc = (n_chunks + 255) / 256;
    KZG_MARK(6);
    hipLaunchKernelGGL(k_red_chunk_sums, dim3(gc), dim3(256), 0, st, ws.bucket.as<int32_t>(), (size_t)p.G, n_chunks, p.m,
                       ws.chunkS.as<int32_t>(), (size_t)n_chunks);
    hipLaunchKernelGGL(k_red_suffix_scan, dim3(n_windows), dim3(p.T), 0, st, ws.chunkS.as<int32_t>(), ws.chunkTmp.as<int32_t>(),
                       (size_t)n_chunks, p.T);
    hipLaunchKernelGGL(k_red_chunk_running, dim3(gc), dim3(256), 0, st, ws.bucket.as<int32_t>(), (size_t)p.G,
                       ws.chunkS.as<int32_t>(), (size_t)n_chunks, n_chunks, p.T, p.m, ws.chunkA.as<int32_t>());
    hipLaunchKernelGGL(k_red_window_sum, dim3(n_windows), dim3(p.T), 0, st, ws.chunkA.as<int32_t>(), (size_t)n_chunks, p.T,
                       L.d_out);
    return KZG_OK;
}

// partial sums -> the p.n_out result points in the pinned buffer; profiling events 6 (behind the first level) and 7
static int32_t enqueue_reduce(const Launch& L) {
    const int32_t rc = L.p.bitsum ? reduce_bitsum(L) : L.p.tables ? reduce_tables(L) : reduce_generic(L);
    if (rc != KZG_OK) return rc;
    KZG_MARK(7);
    return KZG_OK;
}
#undef KZG_MARK

static PlanContext plan_context(const kzg_ctx* ctx) {
    PlanContext pc;
    pc.msm_c_override = ctx->msm_c_override;
    pc.msm_seg_override = ctx->msm_seg_override;
    pc.reduction_lanes = ctx->reduction_lanes;
    pc.acc_wave_slots = ctx->acc_wave_slots;
    for (int sl = 0; sl < KZG_NUM_SLOTS; ++sl) pc.other_in_flight |= ctx->slot_pending[sl] != nullptr;
    return pc;
}

static DeviceBuffer* ws_buffer(MsmWorkspace& ws, int which) {
    DeviceBuffer* const buffers[WS_BUFFERS] = {&ws.digits, &ws.sorted, &ws.count, &ws.sort_tmp, &ws.sort_key, &ws.sort_small, &ws.blockbase, &ws.offs, &ws.block_sums,
                                               &ws.head, &ws.cont, &ws.bucket, &ws.chunkS, &ws.chunkTmp, &ws.chunkA};      // (the order of WsBuffer)
    return buffers[which];
}
// the workspace's pinned result buffer (MSM_MAX_OUT G1 XYZZ values + the entry counts of profiled launches), allocated on first use
int32_t msm_pinned_out(kzg_ctx* ctx, MsmWorkspace& ws) {
    if (ws.pinned_out) return KZG_OK;
    KZG_HIP_TRY(ctx, hipHostMalloc(&ws.pinned_out, (size_t)MSM_MAX_OUT * 32 * 4 + MSM_MAX_PARTS * 4, hipHostMallocDefault));
    KZG_HIP_TRY(ctx, hipHostGetDevicePointer(&ws.pinned_out_dev, ws.pinned_out, 0));
    return KZG_OK;
}
// Digits and counting sort of generic-mode scalar sets on `st` for the G2 driver (g2msm.hip), whose kernels add points of another
// type: ws.sorted and ws.offs as enqueue_sort leaves them (entries index | sign << 31 grouped by bucket, p.G + 1 offsets).  p: a plan
// of make_plan without tables, with batch 1 or -- p.batch sets of p.n scalars one after the other, all over the same bases -- marked
// shared_bases (every entry then holds its in-set index); only the buffers of the sort are reserved.
int32_t msm_sort_generic(kzg_ctx* ctx, MsmWorkspace& ws, hipStream_t st, const uint4* d_scalars, const Plan& p) {
    if (p.tables || p.bitsum || p.batch == 0 || (p.batch != 1 && !p.shared_bases)) return KZG_ERR_INVALID_ARG;
    for (int i : {WS_DIGITS, WS_SORTED, WS_COUNT, WS_BLOCKBASE, WS_OFFS, WS_BLOCK_SUMS}) KZG_HIP_TRY(ctx, ws_buffer(ws, i)->reserve(p.bytes[i]));
    const MsmBases none;
    const Launch L{ctx, ws, st, none, d_scalars, p, nullptr, false};
    const int32_t rc = enqueue_sort(L, nullptr);
    if (rc != KZG_OK) return rc;
    KZG_HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

// Enqueue every kernel of one MSM (or batch) on `st`, using `ws`: plan, validate, reserve, sort, accumulate, reduce.
static int32_t msm_enqueue(kzg_ctx* ctx, MsmWorkspace& ws, hipStream_t st, const MsmBases& bases, const uint4* d_scalars, size_t n,
                           uint32_t batch, Pending* pend, uint32_t out_off = 0, uint32_t out_cap = MSM_MAX_OUT, uint32_t polys = 0,
                           const PolyPtrs* poly_ptrs = nullptr) {
    const Plan p = make_plan(plan_context(ctx), n, bases, batch, polys);
    {
        const char* error = nullptr;
        const int32_t rc = msm_plan_status(p, bases, polys, out_off, out_cap, &error);
        if (error) ctx->last_error = error;
        if (rc != KZG_OK) return rc;
    }
    for (int i = 0; i < WS_BUFFERS; ++i) KZG_HIP_TRY(ctx, ws_buffer(ws, i)->reserve(p.bytes[i]));
    { const int32_t rc = msm_pinned_out(ctx, ws); if (rc != KZG_OK) return rc; }
    // The last kernel of the sequence stores the O(200) result points straight into the pinned host buffer (coherent host memory, read
    // after the event behind that kernel).  A device-to-host copy of them cost ~10 us per MSM -- and above ~16 KiB (208 points at 2^16
    // buckets: every batched launch) hipMemcpyAsync takes the SDMA path, whose set-up after a device-wide synchronisation blocked the
    // enqueueing thread for 5.6-7 ms (gone with HSA_ENABLE_SDMA=0).
    const Launch L{ctx, ws, st, bases, d_scalars, p, reinterpret_cast<uint32_t*>(ws.pinned_out_dev) + (size_t)out_off * 32, ctx->profiling};
    if (L.prof && !ws.ev_ready) {
        for (auto& e : ws.ev) KZG_HIP_TRY(ctx, hipEventCreate(&e));
        ws.ev_ready = true;
    }
    int32_t rc;
    RoctxPhases phases;
    phases.begin(p.bitsum ? "kzg:msm:bit sums" : "kzg:msm:sort");
    if ((rc = enqueue_sort(L, poly_ptrs)) != KZG_OK) return rc;
    if (!p.bitsum) phases.begin("kzg:msm:accumulate");
    if ((rc = enqueue_accumulate(L)) != KZG_OK) return rc;
    if (!p.bitsum) phases.begin("kzg:msm:bucket reduction");
    if ((rc = enqueue_reduce(L)) != KZG_OK) return rc;
    phases.end();
    KZG_HIP_TRY(ctx, hipGetLastError());
    if (L.prof) {                                           // sorted entries = mixed additions of this launch (NAF mode: data dependent; bit sums: none)
        char* slot = static_cast<char*>(ws.pinned_out) + (size_t)MSM_MAX_OUT * 128 + (out_off / MSM_PART_OUT) * 4;
        if (p.bitsum) *reinterpret_cast<uint32_t*>(slot) = 0;
        else KZG_HIP_TRY(ctx, hipMemcpyAsync(slot, ws.offs.as<uint32_t>() + p.G, 4, hipMemcpyDeviceToHost, st));
    }
    if (!ws.ev_done) KZG_HIP_TRY(ctx, hipEventCreateWithFlags(&ws.ev_done, hipEventDisableTiming));
    KZG_HIP_TRY(ctx, hipEventRecord(ws.ev_done, st));        // msm_finish waits for THIS launch, not for the stream: a later MSM may already be queued behind it
    pend->p = p;
    pend->out_off = out_off;
    pend->profiled = true;
    return KZG_OK;
}

static int32_t msm_finish(kzg_ctx* ctx, MsmWorkspace& ws, hipStream_t st, const Pending& pend, kzg_host::Xyzz* result) {
    const Plan& p = pend.p;
    (void)st;
    {
        RoctxRange range_wait("kzg:msm:wait");
        KZG_HIP_TRY(ctx, hipEventSynchronize(ws.ev_done));
    }
    RoctxRange range_epi("kzg:msm:host epilogue");
    if (ctx->profiling && ws.ev_ready && pend.profiled) {
        for (int i = 0; i < 7; ++i) {
            float ms = 0;
            KZG_HIP_TRY(ctx, hipEventElapsedTime(&ms, ws.ev[i], ws.ev[i + 1]));
            ws.phase_ms[i] += ms;
        }
        float ms = 0;
        KZG_HIP_TRY(ctx, hipEventElapsedTime(&ms, ws.ev[0], ws.ev[7]));
        ws.phase_ms[7] += ms;
        ws.profiled_launches += 1;
        ws.profiled_pairs += (uint64_t)p.n * p.batch;
        ws.profiled_entries += reinterpret_cast<const uint32_t*>(static_cast<const char*>(ws.pinned_out) + (size_t)MSM_MAX_OUT * 128)[pend.out_off / MSM_PART_OUT];
    }

    // host epilogue on O(100) points
    using kzg_host::Xyzz;
    static thread_local std::vector<Xyzz> vals_store;
    if (vals_store.size() < p.n_out) vals_store.resize(p.n_out);
    Xyzz* vals = vals_store.data();
    const uint64_t* w = reinterpret_cast<const uint64_t*>(ws.pinned_out) + 16 * (size_t)pend.out_off;
    for (uint32_t i = 0; i < p.n_out; ++i) memcpy(&vals[i], w + 16 * i, 128);
    // The MSMs of a generic batch -- the three linear combinations of batch verification -- take their Horner sums side by side on the host pool
    // (round 6: 0.31 -> 0.11 ms of the 1.7 ms verification core)
    if (!p.tables && p.batch > 1) host_parallel_for(p.batch, [&](size_t b) { result[b] = msm_result(p, vals, p.n_out, (uint32_t)b); });
    else msm_epilogue(p, vals, p.n_out, result);
    return KZG_OK;
}
// n XYZZ results -> affine wire points, and the identity flags where the caller wants them (the identity's wire form is all zero)
static void batch_to_affine(const kzg_host::Xyzz* res, size_t n, uint64_t* out_xy, uint8_t* out_inf) {
    kzg_host::xyzz_batch_to_affine(res, n, out_xy);
    if (!out_inf) return;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t* q = out_xy + 8 * i;
        out_inf[i] = (q[0] | q[1] | q[2] | q[3] | q[4] | q[5] | q[6] | q[7]) == 0 ? 1 : 0;
    }
}
// the synchronous calls share slot 0's workspace and result buffer
static bool slot0_in_flight(kzg_ctx* ctx) {
    if (!ctx->slot_pending[0]) return false;
    ctx->last_error = "a kzg_*_begin on slot 0 is still in flight: call kzg_msm_g1_srs_end(ctx, 0, ..) first";
    return true;
}

// ---- two-slot asynchronous form: begin enqueues, end waits and runs the host epilogue ---------------------------------
// all launches of one MSM of n <= MSM_MAX_LAUNCH pairs on `st` / `ws`
static int32_t msm_enqueue_parts(kzg_ctx* ctx, MsmWorkspace& ws, hipStream_t st, const MsmBases& bases, const uint4* d_scalars, size_t n,
                                 MsmPending* mp) {
    const size_t chunk = msm_launch_len(bases);
    const size_t parts = (n + chunk - 1) / chunk;
    if (parts > MSM_MAX_PARTS) return KZG_ERR_TOO_LARGE;
    mp->n_parts = 0;
    for (size_t k = 0, off = 0; off < n; off += chunk, ++k) {
        MsmBases b = bases;
        b.points = bases.points + 4 * off;
        int32_t rc = msm_enqueue(ctx, ws, st, b, d_scalars + 2 * off, std::min(chunk, n - off), 1, &mp->part[k], parts > 1 ? (uint32_t)k * MSM_PART_OUT : 0u,
                                 parts > 1 ? MSM_PART_OUT : MSM_MAX_OUT);
        if (rc != KZG_OK) { if (k) (void)hipStreamSynchronize(st); return rc; }
        if (k) mp->part[k - 1].profiled = false;
        mp->n_parts = (uint32_t)k + 1;
    }
    return KZG_OK;
}
static int32_t msm_finish_parts(kzg_ctx* ctx, MsmWorkspace& ws, hipStream_t st, const MsmPending& mp, kzg_host::Xyzz* total) {
    *total = kzg_host::xyzz_inf();
    for (uint32_t k = 0; k < mp.n_parts; ++k) {
        kzg_host::Xyzz part;
        int32_t rc = msm_finish(ctx, ws, st, mp.part[k], &part);
        if (rc != KZG_OK) return rc;
        *total = k ? kzg_host::xyzz_add(*total, part) : part;
    }
    return KZG_OK;
}

int32_t msm_slot_stream(kzg_ctx* ctx, int slot, hipStream_t* out) {
    if (slot < 0 || slot >= KZG_NUM_SLOTS) return KZG_ERR_INVALID_ARG;
    // One stream per slot.  How much a third / fourth MSM in flight gains depends on how HIP maps the streams onto its hardware
    // queues (4 by default, shared with every other stream of the process): at 2^17 pairs per MSM, depth 2 gives 0.43-0.45 ms per
    // MSM, depth 3 0.37-0.38 (0.5 in one mapping), depth 4 anything from 0.34 to 0.46.  Sharing streams between slots (2 or 3
    // streams for 4 slots, any assignment) made depth 4 mapping-independent but no faster than depth 2-3 (tools/queue_probe.py).
    if (slot == 0) { *out = ctx->stream; return KZG_OK; }
    if (!ctx->stream_x[slot - 1]) KZG_HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->stream_x[slot - 1], hipStreamNonBlocking));
    *out = ctx->stream_x[slot - 1];
    return KZG_OK;
}

int32_t msm_begin(kzg_ctx* ctx, int slot, const MsmBases& bases, const void* d_scalars, size_t n) {
    if (slot < 0 || slot >= KZG_NUM_SLOTS || ctx->slot_pending[slot]) return KZG_ERR_INVALID_ARG;     // slot still in flight
    if (n == 0) return KZG_ERR_INVALID_ARG;
    if (n > 4 * MSM_MAX_LAUNCH) return KZG_ERR_TOO_LARGE;             // 2^26 pairs: MSM_MAX_PARTS launches of 2^20 (table mode) or four of 2^24
    hipStream_t st = nullptr;
    { int32_t rc0 = msm_slot_stream(ctx, slot, &st); if (rc0 != KZG_OK) return rc0; }
    MsmPending* pend = new (std::nothrow) MsmPending();
    if (!pend) return KZG_ERR_DEVICE;
    int32_t rc = msm_enqueue_parts(ctx, ctx->slot_msm(slot), st, bases, reinterpret_cast<const uint4*>(d_scalars), n, pend);
    if (rc != KZG_OK) { delete pend; return rc; }
    ctx->slot_pending[slot] = pend;
    return KZG_OK;
}

int32_t msm_end(kzg_ctx* ctx, int slot, uint64_t out_xy[8], uint8_t* out_inf, uint64_t* out_xyzz) {
    if (slot < 0 || slot >= KZG_NUM_SLOTS || !ctx->slot_pending[slot]) return KZG_ERR_INVALID_ARG;    // nothing in flight
    MsmPending* pend = ctx->slot_pending[slot];
    if (pend->n_parts && pend->part[0].p.polys) return KZG_ERR_INVALID_ARG;                            // a batched launch: kzg_msm_g1_srs_end_batch collects it
    ctx->slot_pending[slot] = nullptr;
    kzg_host::Xyzz total;
    hipStream_t st = nullptr;
    (void)msm_slot_stream(ctx, slot, &st);
    int32_t rc = msm_finish_parts(ctx, ctx->slot_msm(slot), st, *pend, &total);
    delete pend;
    if (rc != KZG_OK) return rc;
    if (out_xyzz) memcpy(out_xyzz, &total, 128);
    if (out_xy) kzg_host::xyzz_to_affine(total, out_xy, out_inf);
    return KZG_OK;
}

// Asynchronous form of ONE batched launch: `count` polynomials of n scalars each (separate device buffers) over the same per-bit
// tables on `slot`; msm_end_batch waits and returns count results (affine and / or XYZZ partials).
int32_t msm_begin_batch(kzg_ctx* ctx, int slot, const MsmBases& bases, const void* const* d_scalars, size_t n, size_t count) {
    if (slot < 0 || slot >= KZG_NUM_SLOTS || ctx->slot_pending[slot]) return KZG_ERR_INVALID_ARG;
    if (!bases.naf || n == 0 || count == 0 || count > (size_t)MSM_BATCH_PTRS || count > msm_batch_capacity(n)) return KZG_ERR_INVALID_ARG;
    hipStream_t st = nullptr;
    { int32_t rc0 = msm_slot_stream(ctx, slot, &st); if (rc0 != KZG_OK) return rc0; }
    MsmPending* pend = new (std::nothrow) MsmPending();
    if (!pend) return KZG_ERR_DEVICE;
    PolyPtrs ptrs{};
    for (size_t k = 0; k < count; ++k) ptrs.p[k] = reinterpret_cast<const uint4*>(d_scalars[k]);
    int32_t rc = msm_enqueue(ctx, ctx->slot_msm(slot), st, bases, ptrs.p[0], n * count, 1, &pend->part[0], 0, MSM_MAX_OUT, (uint32_t)count, &ptrs);
    if (rc != KZG_OK) { delete pend; return rc; }
    pend->n_parts = 1;
    ctx->slot_pending[slot] = pend;
    return KZG_OK;
}
int32_t msm_end_batch(kzg_ctx* ctx, int slot, size_t count, uint64_t* out_xy, uint8_t* out_inf, uint64_t* out_xyzz) {
    if (slot < 0 || slot >= KZG_NUM_SLOTS || !ctx->slot_pending[slot]) return KZG_ERR_INVALID_ARG;
    MsmPending* pend = ctx->slot_pending[slot];
    if (pend->n_parts != 1 || pend->part[0].p.polys != count) return KZG_ERR_INVALID_ARG;       // (not a batched launch of that size: left in flight)
    ctx->slot_pending[slot] = nullptr;
    static thread_local std::vector<kzg_host::Xyzz> res;
    res.resize(count);
    hipStream_t st = nullptr;
    (void)msm_slot_stream(ctx, slot, &st);
    int32_t rc = msm_finish(ctx, ctx->slot_msm(slot), st, pend->part[0], res.data());
    delete pend;
    if (rc != KZG_OK) return rc;
    if (out_xyzz) memcpy(out_xyzz, res.data(), count * 128);
    if (out_xy) batch_to_affine(res.data(), count, out_xy, out_inf);
    return KZG_OK;
}

#ifdef KZG_ACC_STAMPS
}  // namespace kzg
// diagnostic build only: per-wave {start, end (100 MHz ticks), HW_ID, XCC_ID} of the last accumulate launch of slot 0
extern "C" int32_t kzg_debug_acc_stamps(kzg_ctx* ctx, uint64_t* out, size_t n_waves, size_t nl) {
    if (hipMemcpy(out, static_cast<const char*>(ctx->msm.cont.p) + nl * 36 * 4, n_waves * 64, hipMemcpyDeviceToHost) != hipSuccess) return -3;
    return 0;
}
namespace kzg {
#endif

void msm_drop_slots(kzg_ctx* ctx) {
    for (int s = 0; s < KZG_NUM_SLOTS; ++s) { delete ctx->slot_pending[s]; ctx->slot_pending[s] = nullptr; }
}

int32_t points_wire_to_device(kzg_ctx* ctx, const uint4* d_wire, uint4* d_out, size_t n, uint32_t* d_off_curve_flag) {
    if (n == 0) return KZG_OK;
    if (d_off_curve_flag) hipLaunchKernelGGL(k_points_wire_to_device_checked, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_wire, d_out, n, d_off_curve_flag);
    else hipLaunchKernelGGL(k_points_wire_to_device, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_wire, d_out, n);
    KZG_HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

// Negative result kept for the record (measured on MI355X at 2^20, removed from the code): cutting one large table-mode MSM
// in two halves on two streams, so that the sort / bucket reduction of one half runs beside the accumulate of the other, took
// 2.36 ms against 2.09 ms unsplit -- inside ONE MSM the halves' small kernels stretch 3-4x and the accumulates slow each other.
// Overlap pays across INDEPENDENT MSMs instead (the two slots below).
int32_t msm_run(kzg_ctx* ctx, const MsmBases& bases, const void* d_scalars, size_t n,
                uint64_t out_xy[8], uint8_t* out_inf, uint64_t* out_xyzz) {
    if (slot0_in_flight(ctx)) return KZG_ERR_INVALID_ARG;
    kzg_host::Xyzz total = kzg_host::xyzz_inf();
    const uint4* sc = reinterpret_cast<const uint4*>(d_scalars);
    static thread_local MsmPending mp;
    for (size_t off = 0; off < n; off += MSM_MAX_LAUNCH) {
        const size_t len = std::min(MSM_MAX_LAUNCH, n - off);
        MsmBases b = bases;
        b.points = bases.points + 4 * off;
        kzg_host::Xyzz part;
        int32_t rc = msm_enqueue_parts(ctx, ctx->msm, ctx->stream, b, sc + 2 * off, len, &mp);
        if (rc == KZG_OK) rc = msm_finish_parts(ctx, ctx->msm, ctx->stream, mp, &part);
        if (rc != KZG_OK) return rc;
        total = off ? kzg_host::xyzz_add(total, part) : part;
    }
    if (out_xyzz) memcpy(out_xyzz, &total, 128);
    if (out_xy) kzg_host::xyzz_to_affine(total, out_xy, out_inf);
    return KZG_OK;
}

// `batch` independent MSMs of n pairs each over concatenated caller bases (generic mode): one kernel sequence.
int32_t msm_run_batch(kzg_ctx* ctx, const uint4* d_points, const void* d_scalars, size_t n, uint32_t batch,
                      uint64_t* out_xy /* batch x 8 */, uint8_t* out_inf /* batch */) {
    if (n > MSM_MAX_LAUNCH / batch) return KZG_ERR_TOO_LARGE;
    if (slot0_in_flight(ctx)) return KZG_ERR_INVALID_ARG;
    MsmBases b;
    b.points = d_points;
    kzg_host::Xyzz res[64];
    if (batch > 64) return KZG_ERR_INVALID_ARG;
    Pending pend;
    int32_t rc = msm_enqueue(ctx, ctx->msm, ctx->stream, b, reinterpret_cast<const uint4*>(d_scalars), n, batch, &pend);
    if (rc == KZG_OK) rc = msm_finish(ctx, ctx->msm, ctx->stream, pend, res);
    if (rc != KZG_OK) return rc;
    for (uint32_t i = 0; i < batch; ++i) kzg_host::xyzz_to_affine(res[i], out_xy + 8 * i, out_inf ? out_inf + i : nullptr);
    return KZG_OK;
}

// `polys` MSMs of n pairs each over the SAME bases (the first n points of an SRS with per-bit tables): the commitments of `polys`
// polynomials in one kernel sequence per MSM_BATCH_POLYS_MAX polynomials.  d_scalars: polys x n wire scalars, polynomial after polynomial.
int32_t msm_run_batch_tables(kzg_ctx* ctx, const MsmBases& bases, const void* d_scalars, size_t n, size_t polys, uint64_t* out_xy, uint8_t* out_inf) {
    if (!bases.naf || n == 0) return KZG_ERR_INVALID_ARG;
    for (int sl = 0; sl < KZG_NUM_SLOTS; ++sl)
        if (ctx->slot_pending[sl]) {
            ctx->last_error = "a kzg_*_begin is still in flight: the batched commitments use the slots' streams and workspaces themselves";
            return KZG_ERR_INVALID_ARG;
        }
    const size_t per = msm_batch_capacity(n);              // polynomials per launch
    if (per == 0) return KZG_ERR_TOO_LARGE;
    // The launches run as a software pipeline over the slots (their own streams and workspaces): launch k + 1 .. k + 2 are enqueued
    // before launch k is collected, so the latency-bound kernels of one overlap the accumulate kernel of another -- a launch of 2^17
    // scalars takes 0.42 ms alone and 0.22 ms with three in flight (section 6b of DESIGN.md).
    constexpr int DEPTH = 3;
    static_assert(DEPTH <= KZG_NUM_SLOTS, "one slot per launch in flight");
    Pending pend[DEPTH];
    size_t first[DEPTH] = {}, cnt[DEPTH] = {};
    bool busy[DEPTH] = {};
    static thread_local std::vector<kzg_host::Xyzz> res;
    res.resize(std::min(per, polys));
    const uint4* sc = reinterpret_cast<const uint4*>(d_scalars);
    auto collect = [&](int s) -> int32_t {
        hipStream_t st = nullptr;
        (void)msm_slot_stream(ctx, s, &st);
        int32_t rc = msm_finish(ctx, ctx->slot_msm(s), st, pend[s], res.data());
        busy[s] = false;
        if (rc != KZG_OK) return rc;
        batch_to_affine(res.data(), cnt[s], out_xy + 8 * first[s], out_inf ? out_inf + first[s] : nullptr);
        return KZG_OK;
    };
    int32_t rc = KZG_OK;
    size_t launch = 0;
    for (size_t done = 0; done < polys && rc == KZG_OK; done += per, ++launch) {
        const int s = (int)(launch % DEPTH);
        if (busy[s]) rc = collect(s);
        if (rc != KZG_OK) break;
        const size_t k = std::min(per, polys - done);
        hipStream_t st = nullptr;
        rc = msm_slot_stream(ctx, s, &st);
        if (rc != KZG_OK) break;
        rc = msm_enqueue(ctx, ctx->slot_msm(s), st, bases, sc + 2 * done * n, n * k, 1, &pend[s], 0, MSM_MAX_OUT, (uint32_t)k);
        if (rc != KZG_OK) break;
        first[s] = done; cnt[s] = k; busy[s] = true;
    }
    for (size_t q = 0; q < DEPTH; ++q) {                   // drain in launch order (also after an error: nothing stays in flight)
        const int s = (int)((launch + q) % DEPTH);
        if (!busy[s]) continue;
        const int32_t r2 = collect(s);
        if (rc == KZG_OK) rc = r2;
    }
    return rc;
}

}  // namespace kzg

#if defined(KZG_TEST_HOOKS)           // libkzg_bn254_mi355x_hooks.so only (make hooks; tests/test_gpu_accumulate_replay.py)
// partial sums that k_msm_accumulate recomputed with the checked addition since the last reset (device-wide; call with no MSM in flight)
extern "C" int kzg_test_acc_replays(unsigned long long* out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(kzg::g_acc_replays), sizeof(unsigned long long)) != hipSuccess) return -1;
    const unsigned long long zero = 0;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(kzg::g_acc_replays), &zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
#endif

#if defined(KZG_DEVICE_BOUND_CHECK)   // the device bound-check variant only (field29.h, `make boundcheck`)
#include "field29.h"
KZG_BOUND_CHECK_EXPORTS(msm)
#endif
