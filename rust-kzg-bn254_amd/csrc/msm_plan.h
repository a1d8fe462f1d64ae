// msm_plan.h — the planner of the G1 MSM driver (msm.hip): from the length, the bases' shape and four context settings to everything the
// driver decides before its first launch -- mode, window bits, grids, sort form, reduction lane group, result points, workspace bytes --
// and the one function that accepts or rejects the launch.  Pure host code: no HIP type, no kzg_ctx; also compiled with g++ by
// tests/hostcheck/plancheck.cpp, which pins every plan of a fixed grid (tests/golden/msm_plans.txt).
// The comments that quote measurements are the record of why a threshold has its value.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "../../include/kzg_bn254_mi355x.h"
#include "msm_limits.h"
#include "naf.h"

namespace kzg {

// The part of an MSM's bases the planner reads (engine.h MsmBases adds the points): table_stride > 0 selects the precomputed-table mode
// (tables `table_stride` points apart, window bits c, W tables).
struct MsmBasesShape {
    uint32_t table_stride = 0;
    int c = 0;
    int W = 0;
    bool bitsum = false;  // tiny MSM: `points` = the per-bit tables, summed directly (k_bitsum_level1 / 2, msm_kernels.h section 6e)
    bool naf = false;     // `points` = the per-bit tables (Bit_j[i] = 2^j P_i, j < 255, table_stride points apart): width-(c + 1) NAF digits
};

// The part of a context the planner reads (kzg_ctx, engine.h)
struct PlanContext {
    int msm_c_override = 0;
    int msm_seg_override = 0;
    int reduction_lanes = 0;
    uint32_t acc_wave_slots = 3 * 1024;
    bool other_in_flight = false;   // some slot of the context has an MSM in flight
};

// the workspace buffers of one launch (MsmWorkspace, engine.h), in the order the driver reserves them
enum WsBuffer { WS_DIGITS, WS_SORTED, WS_COUNT, WS_SORT_TMP, WS_SORT_KEY, WS_SORT_SMALL, WS_BLOCKBASE, WS_OFFS, WS_BLOCK_SUMS, WS_HEAD, WS_CONT, WS_BUCKET,
                WS_CHUNK_S, WS_CHUNK_TMP, WS_CHUNK_A, WS_BUFFERS };

inline int ilog2_floor(size_t n) { int k = 0; while ((n >> (k + 1)) != 0) ++k; return k; }

struct Plan {
    uint32_t n;          // pairs per MSM in this launch
    uint32_t batch;      // independent MSMs of n pairs each (generic mode only; 1 otherwise)
    bool shared_bases = false;   // generic mode, batch > 1: every MSM of the batch reads the SAME n bases, so a sorted entry holds the in-MSM
                                 // index i < n, not msm * n + i (the G2 driver's batches, g2msm_plan.h; set by the caller of make_plan)
    bool tables;         // table mode
    bool naf;            // table mode over the per-bit tables: width-(c + 1) NAF digits (msm_kernels.h), W = most entries per scalar
    uint32_t polys;      // BATCHED table mode (NAF, c = 7): the n scalars are `polys` polynomials of n / polys coefficients over the same bases,
                         // 64 buckets each: B = 64 polys buckets, one group of the first reduction level per polynomial (0: one MSM)
    int c, W;
    uint32_t B;          // buckets per set
    uint32_t sets;       // bucket sets (1 in table mode, W otherwise)
    uint32_t G;          // sets * B
    uint32_t nl;         // lanes of the accumulate kernel (a multiple of 256); each adds ceil(E / nl) sorted entries
    uint32_t set_len;    // digit entries per set
    uint32_t tile_len, tiles_per_set, tiles;
    bool bitsum;         // tiny MSM over the per-bit tables as a plain sum (k_bitsum_level1 / 2): n_out <= 8 result points for the host to add
    bool fused;          // sparse table-mode MSM: the first reduction level adds the sorted entries itself; its group g holds the buckets gp * G1 + g
    bool quad;           // reduction levels on lane quads (curve_quad.h): no other MSM in flight when this one was planned
    bool alone = false;  // planned with no other MSM of this context in flight
    bool sort2;          // two-level sort (table mode, index fits 24 bits)
    bool sort_small;     // global-atomic sort (few entries)
    uint32_t Hb, tile1, tiles1, tiles2cap;
    uint32_t T, m;       // generic-mode reduction: chunks per window, buckets per chunk
    // table mode: a sorted entry holds window * idx_stride + i.  idx_stride = the table stride, or (compact form, SRS of more than
    // 2^20 points) the next power of two >= n, 2^idx_log, with the accumulate kernel adding window * stride_adj
    uint32_t idx_stride, idx_log, stride_adj;
    int ND;              // digit words per scalar (NAF sort)
    bool lean_sort;      // small table-mode MSM (one bucket set): digits + histogram in one pass, one-workgroup scan, scatter
    bool quad1;          // the FIRST reduction level on lane quads (the second follows `quad`)
    int bitsum_chunk;    // bit sums: positions per quad (8 / 16 / 32) ...
    uint32_t bitsum_wg;  // ... and workgroups of the first launch
    uint32_t n_out;      // wire XYZZ values the last kernel leaves for the host epilogue
    size_t bytes[WS_BUFFERS];   // what each workspace buffer must hold (0: not used)

    uint32_t G1() const { return B / 64; }                       // groups of 64 buckets: workgroups of the first reduction level
    uint32_t G1p() const { return (G1() + 63) / 64; }            // units of 4 096 buckets
    uint32_t n_windows() const { return (uint32_t)W * batch; }   // window sums produced in generic mode
    uint32_t n_chunks() const { return n_windows() * T; }
    uint32_t scan_blocks() const { return (G + SCAN_TILE - 1) / SCAN_TILE; }
    size_t entries() const { return (size_t)W * n * batch; }     // most sorted entries (NAF: the count is only known on the device)
};

// Window bits of the generic mode for `batch` MSMs of n pairs: W * batch window sums leave the device (<= MSM_MAX_OUT).
inline int generic_window(size_t n, uint32_t batch) {
    int c = std::min(14, std::max(4, ilog2_floor(n) - 6));
    while (c < 16 && (size_t)((255 + c - 1) / c) * batch > MSM_MAX_OUT) ++c;
    return c;
}

// Batched table mode: bucket bits per polynomial by its length (width c + 1 digits over the per-bit tables).  Short polynomials: 64
// buckets, one group of the first reduction level each; from 2^13 coefficients whole units of 4 096 buckets, reduced like a single MSM.
inline int batch_bucket_bits(size_t poly_len) {
    if (poly_len < ((size_t)1 << 13)) return 7;
    if (poly_len < ((size_t)1 << 15)) return 13;
    if (poly_len < ((size_t)1 << 18)) return 15;
    return 16;
}

// Pairs per launch of an MSM over `bases`.  Tables more than 2^24 / W points apart (an SRS beyond 2^20 points at c = 17) are walked
// in power-of-two chunks whose COMPACT indices fit the two-level sort (make_plan): a 2^22-point commitment is four 2^20 launches.
inline size_t msm_launch_len(const MsmBasesShape& bases) {
    if (bases.naf) return MSM_MAX_LAUNCH;
    if (bases.table_stride != 0 && (size_t)bases.W * bases.table_stride > ((size_t)1 << SORT2_IDX_BITS)) {
        size_t cpow = 1;
        while (((size_t)bases.W * cpow * 2) <= ((size_t)1 << SORT2_IDX_BITS)) cpow *= 2;
        if (cpow >= ((size_t)1 << 16)) return cpow;
    }
    return MSM_MAX_LAUNCH;
}

// polynomials one batched launch takes (batched table mode): 2^(c-1) buckets each in one 2^16-bucket array, 2^24 pairs at most
inline size_t msm_batch_capacity(size_t n) {
    if (n == 0) return 0;
    const int cb = batch_bucket_bits(n);
    return std::min<size_t>(std::min<size_t>(MSM_BATCH_POLYS_MAX, (size_t)65536 >> (cb - 1)), MSM_MAX_LAUNCH / n);
}

// tiny MSM: two launches, n_out result points (msm_kernels.h section 6e)
inline Plan bitsum_plan(size_t n) {
    Plan p{};
    p.n = (uint32_t)n; p.batch = 1; p.tables = true; p.bitsum = true; p.B = 64; p.G = 64; p.W = 255; p.c = 7;
    p.bitsum_chunk = n <= 512 ? 8 : n <= 2048 ? 16 : 32;                     // positions per quad: one wave per SIMD at 512 / 1 024 scalars (the six-step tree of every workgroup is what the launch costs: 2^9 30 us with 8, 38 with 4; 2^11 63 with 16, 77 with 8)
    p.bitsum_wg = (uint32_t)((n * (size_t)(256 / p.bitsum_chunk) + 63) / 64);
    p.n_out = (p.bitsum_wg + 63) / 64;                 // <= 8 points for the host to add
    p.bytes[WS_CHUNK_S] = (size_t)p.bitsum_wg * 36 * 4;
    return p;
}

// Total: every input gives a plan that msm_plan_status can judge (a polys count it rejects is planned as one MSM).
inline Plan make_plan(const PlanContext& ctx, size_t n, const MsmBasesShape& bases, uint32_t batch, uint32_t polys = 0) {
    if (bases.bitsum && batch == 1 && !polys && n <= BITSUM_MAX_N) return bitsum_plan(n);
    Plan p{};
    p.n = (uint32_t)n;
    p.batch = batch;
    p.tables = bases.table_stride != 0;
    p.naf = p.tables && bases.naf;
    p.polys = p.naf && polys <= MSM_BATCH_POLYS_MAX ? polys : 0;
    // lane quads for the two reduction levels when this MSM runs alone (0.7 of the pair form's dependent instructions, twice its lanes);
    // with another MSM in flight the SIMDs are shared and the pair form's fewer instructions count (kzg_ctx_set_reduction_lanes forces either).
    p.quad = p.tables && !ctx.other_in_flight;
    if (ctx.reduction_lanes) p.quad = p.tables && ctx.reduction_lanes == 4;
    p.alone = !ctx.other_in_flight;
    int c;
    if (p.polys) {
        c = batch_bucket_bits(n / p.polys);                // 7: 64 buckets per polynomial (k_batch_finish); 13 / 15 / 16: whole units of 4 096 buckets (second level + host epilogue per polynomial)
    } else if (p.tables) {
        c = bases.c;
        // NAF mode, 2^18 .. 2^19 - 1 pairs, nothing else in flight (the reference's bench_kzg_commit_8mb shape): 2^14 buckets instead of 2^15 --
        // alone, the reductions cost their latency, not their instructions: 0.551 -> 0.525 ms at 2^18 (with other MSMs in flight 16 stays
        // ahead, engine.h srs_naf_c; tools/archive/sweep_naf_c_alone.py).
        if (p.naf && c == 16 && p.alone && n < ((size_t)1 << 19)) c = 15;
    } else {
        c = ctx.msm_c_override;
        if (c == 0) c = generic_window(n, batch);
        c = std::min(16, std::max(2, c));
    }
    p.c = c;
    p.W = p.naf ? naf_max_digits(c + 1) : (255 + c - 1) / c;
    p.B = p.polys ? (c == 7 ? 64u * ((p.polys + 1u) & ~1u) : p.polys << (c - 1)) : 1u << (c - 1);      // (a multiple of 128: whole coarse bins)
    p.sets = p.tables ? 1u : (uint32_t)p.W * batch;
    p.G = p.sets * p.B;
    const size_t entries_cap = (size_t)p.W * n * batch;                  // buffer sizes
    // NAF: the entry count is only known on the device (offs[G]); 254 / (w + 1) per scalar on average sizes the accumulate grid
    const size_t entries = p.naf ? std::max<size_t>(1, (size_t)((double)n * 254.0 / (double)(c + 2))) : entries_cap;
    {
        // Lanes of the accumulate kernel.  Large MSMs: one full round of resident waves (acc_wave_slots = 3 per SIMD), every
        // lane with the same trip count.  Small MSMs: at least Lmin entries per lane -- short trips keep them from serialising
        // ~100 dependent mixed adds (10 us each) in a handful of waves; from 2^21 entries on, below 24 entries per lane the
        // folding of the lane partials costs more than the extra waves buy (measured in round 1: 15 -> 0.655 ms, 24 -> 0.582 ms).
        const int L = ctx.msm_seg_override;
        size_t lanes;
        if (L > 0) {
            lanes = (entries + (size_t)L - 1) / (size_t)L;                 // forced trip count (tests, sweeps): no cap
        } else {
            const size_t lmin = entries >= ((size_t)1 << 21) ? 24 : 4;
            // Round 3: TWO waves per SIMD (of the three the 168-VGPR kernel could hold) unless this is a large MSM running alone.
            // A grid that fills all three slots leaves no registers for any other kernel on the chip, so the sort and the reductions
            // of the other MSM in flight only ran in the tail of this kernel; with a third of the slots free they run beside it:
            // pipelined step 1.183-1.192 -> 1.160-1.166 ms (same box, 3072 / 2048 wave slots; 2560 = 2.5 waves per SIMD: 1.17-1.18),
            // and below 2^19 pairs fewer lanes also mean fewer partial sums for the first reduction level (2^16: 0.464 -> 0.403 ms,
            // 2^17: 0.534 -> 0.486).  Alone, a 2^19 / 2^20-pair MSM is 2-3 % faster on three (0.929 / 1.474 against 0.961 / 1.496 ms).
            size_t slots = ctx.acc_wave_slots;
            if (ctx.other_in_flight || entries < ((size_t)1 << 23)) slots = slots / 3 * 2;
            // below 2^22 entries (2^15 .. 2^17 pairs; 2^18 is even) ONE wave per SIMD: the kernel is not throughput bound there (the same
            // 0.20 ms at 2^17 pairs with 65 536 lanes of 30 entries as with 131 072 of 15), half the lanes leave half the partial sums
            // to the first reduction level (0.097 -> 0.084 ms) and room for the other MSMs in flight: three in flight 2^15 0.154 ->
            // 0.136, 2^16 0.191 -> 0.160, 2^17 0.245 -> 0.211 ms per MSM (wave-slot sweep, profiles/r03_naf.md)
            if (entries < ((size_t)1 << 22)) slots = ctx.acc_wave_slots / 3;
            lanes = std::min<size_t>(slots * 64, (entries + lmin - 1) / lmin);
        }
        lanes = std::max<size_t>(256, (lanes + 255) / 256 * 256);
        p.nl = (uint32_t)std::min<size_t>(lanes, (size_t)1 << 24);
    }
    p.set_len = (uint32_t)(p.tables ? entries_cap : n);
    p.idx_stride = bases.table_stride; p.idx_log = 31; p.stride_adj = 0;
    if (p.tables && !p.naf && (size_t)p.W * bases.table_stride > ((size_t)1 << SORT2_IDX_BITS)) {
        int lg = ilog2_floor(n);
        if (((size_t)1 << lg) < n) ++lg;
        if (((size_t)p.W << lg) <= ((size_t)1 << SORT2_IDX_BITS) && ((size_t)1 << lg) <= bases.table_stride) {
            p.idx_log = (uint32_t)lg; p.idx_stride = 1u << lg; p.stride_adj = bases.table_stride - p.idx_stride;
        }
    }
    // single-pass sort tiles: large against the bucket count (one contiguous flush of B counters per tile), and not too many
    size_t tile = std::max<size_t>(4096, 2 * (size_t)p.B);
    while (tile < p.set_len && ((size_t)p.set_len + tile - 1) / tile * p.sets > 1024) tile *= 2;   // (many small sets: one tile per set)
    p.tile_len = (uint32_t)tile;
    p.tiles_per_set = (uint32_t)(((size_t)p.set_len + tile - 1) / tile);
    p.tiles = p.tiles_per_set * p.sets;
    {
        const bool lds_fits = (size_t)p.B * 4 <= SORT1_MAX_LDS;            // single-pass sort: one LDS counter per bucket
        p.sort_small = !p.naf && entries < ((size_t)1 << 18);
        const bool can2 = p.tables && (p.c - 1 > SORT2_LO_BITS || p.polys) && (p.B >> SORT2_LO_BITS) <= SORT2_MAX_BINS &&
                          (p.naf ? (size_t)NAF_POSITIONS * p.idx_stride < ((size_t)1 << 31)
                                 : (size_t)p.W * p.idx_stride <= ((size_t)1 << SORT2_IDX_BITS));
        // from 2^18 entries (was 2^23): the scalar-tile pass 1 and the per-bin pass 2 win from the first size the single-pass sort is not "small" for
        p.sort2 = !p.sort_small && can2 && (entries >= ((size_t)1 << 18) || !lds_fits || p.naf);
        if (!p.sort2 && !lds_fits) p.sort_small = true;                    // (slow but correct: a forced odd configuration)
        p.Hb = p.sort2 ? (p.B >> SORT2_LO_BITS) : 0;
        p.tile1 = n >= ((size_t)1 << 19) ? 2048 : 1024;                    // SCALARS per pass-1 tile (W entries each)
        if (p.naf) {                                                       // the recoding is a long dependent chain per scalar: more, smaller tiles
            p.tile1 = 512;
            if (p.polys) p.tile1 = 2048;                                    // (twice the entries per scalar: fewer, larger tiles)
        }
        p.tiles1 = (uint32_t)((n + p.tile1 - 1) / p.tile1);
        p.tiles2cap = (uint32_t)(entries_cap / SORT2_CHUNK + p.Hb + 1);
    }
    p.T = std::min<uint32_t>(p.B, RED_T);
    p.m = p.B / p.T;
    p.ND = p.c + 1 >= 16 ? NAF_DIGITS : 32;        // digit words per scalar (width >= 16: at most 16 digits)
    p.lean_sort = !p.sort2 && p.sort_small && p.tables && batch == 1 && p.G == p.B && p.G <= SCAN1_MAX;
    // the two reduction levels run on lane pairs (curve_pair.h; one 128-thread workgroup per 64 buckets, then per two groups of 64 sums) or lane quads
    // sparse table-mode MSMs (at most 2.5 entries per bucket on average: commitments of <= 2^11 coefficients on
    // the c = 15 tables): the first reduction level adds the entries itself (k_msm_bucket_bits1_fused), there is no accumulate kernel and
    // there are no partial sums.  Measured (tools/phases_small.py, same box, device time of one commitment): 2^8 170 -> 125 us, 2^9 163 -> 128,
    // 2^10 165 -> 152, 2^11 199 -> 195; at 2^12 (4.25 per bucket) 206 -> 261: a wave waits for its fullest bucket, the equal split does not.
    p.fused = p.tables && !p.naf && (double)entries_cap <= 2.5 * (double)p.B;
    // (at 2^16 buckets the unfused level is 4 096 quad waves of ~11 000 instructions: throughput bound, 0.121 against 0.114 ms on pairs)
    p.quad1 = p.quad && (p.fused || p.G1() <= 512 || ctx.reduction_lanes == 4);
    p.n_out = !p.tables ? p.n_windows() : p.polys && p.c == 7 ? p.polys : p.G1() == 1 ? 7 : 13 * p.G1p();

    size_t* by = p.bytes;
    by[WS_SORTED] = entries_cap * 4;
    by[WS_COUNT] = (size_t)p.G * 4 + 16;
    if (p.sort2) {
        by[WS_SORT_TMP] = entries_cap * 4;
        if (p.naf) {
            by[WS_SORT_KEY] = entries_cap + 16;
            by[WS_DIGITS] = (size_t)n * p.ND * 4;
        }
        by[WS_SORT_SMALL] = ((size_t)3 * (p.Hb + 1) + p.tiles2cap) * 4 + 64;
        by[WS_BLOCKBASE] = std::max((size_t)p.tiles1 * p.Hb, (size_t)p.tiles2cap * SORT2_LO) * 4;
    } else {
        by[WS_DIGITS] = entries_cap * 4;
        by[WS_BLOCKBASE] = p.sort_small ? (size_t)p.G * 4 : (size_t)p.tiles * p.B * 4;
    }
    by[WS_OFFS] = ((size_t)p.G + 1) * 4 + 16;
    by[WS_BLOCK_SUMS] = (size_t)SCAN_TILE * 4;
    by[WS_HEAD] = (size_t)p.G * 36 * 4;
    by[WS_CONT] = (size_t)p.nl * 36 * 4;
#ifdef KZG_ACC_STAMPS
    by[WS_CONT] += (size_t)(p.nl / 64) * 64;
#endif
    if (p.tables) {
        by[WS_CHUNK_S] = (size_t)7 * p.G1() * 36 * 4;          // X1
    } else {
        by[WS_BUCKET] = (size_t)p.G * 36 * 4;
        by[WS_CHUNK_S] = by[WS_CHUNK_TMP] = by[WS_CHUNK_A] = (size_t)p.n_chunks() * 36 * 4;
    }
    return p;
}

// KZG_OK, or the status msm_enqueue returns instead of launching, in this order of precedence.  *error: the text for last_error where the
// rejection has one of its own.
inline int32_t msm_plan_status(const Plan& p, const MsmBasesShape& bases, uint32_t polys, uint32_t out_off, uint32_t out_cap, const char** error) {
    *error = nullptr;
    if (p.batch == 0 || (p.batch > 1 && bases.table_stride != 0)) return KZG_ERR_INVALID_ARG;
    if (polys && (!bases.naf || p.n % polys != 0 || polys > MSM_BATCH_POLYS_MAX)) return KZG_ERR_INVALID_ARG;
    if (p.bitsum) return out_cap < p.n_out || out_off + p.n_out > MSM_MAX_OUT ? KZG_ERR_INVALID_ARG : KZG_OK;
    if (p.polys && p.B > 65536) return KZG_ERR_INVALID_ARG;
    if (!p.tables && p.n_windows() > MSM_MAX_OUT) return KZG_ERR_INVALID_ARG;
    if (p.G > SCAN1_MAX && p.scan_blocks() > SCAN_TILE) return KZG_ERR_INVALID_ARG;
    if (p.tables && p.G1() > 1 && 13 * p.G1p() > MSM_MAX_OUT) return KZG_ERR_INVALID_ARG;
    // this launch owns [out_off, out_off + out_cap) of the pinned result buffer (one MSM_PART_OUT window per part of a multi-part MSM)
    if (p.n_out > out_cap || out_off + p.n_out > MSM_MAX_OUT) {
        *error = "MSM result points exceed this launch's window of the result buffer";
        return KZG_ERR_INVALID_ARG;
    }
    return KZG_OK;
}

}  // namespace kzg
