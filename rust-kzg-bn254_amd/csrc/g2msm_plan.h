// g2msm_plan.h — the planner of the G2 MSM driver (g2msm.hip): from the length and the number of base sets to everything the driver
// decides before its first launch -- blobs per launch, window bits, the sort's plan, accumulate lanes, reduction chunks, result points,
// workspace bytes, launches -- and the one function that accepts or rejects.  Pure host code like msm_plan.h: no HIP type, no kzg_ctx; also compiled with
// g++ by tests/hostcheck/g2msm_plancheck.cpp.
//
// The G2 MSM is the bucket method with signed c-bit windows over the bases as given (no precomputed tables): W = ceil(255 / c) bucket
// sets of B = 2^(c-1) buckets.  Digits and counting sort are the generic mode of the G1 driver (msm_plan.h make_plan, msm.hip
// msm_sort_generic): the embedded `sort` plan is exactly what that path launches, so the two drivers cannot disagree about it.
#pragma once
#include "msm_plan.h"

namespace kzg {

constexpr uint32_t G2MSM_MAX_LAUNCH = 1u << 22;   // pairs per launch: W n entries keep 32-bit positions with room (19 * 2^22 < 2^27); longer MSMs run as parts
constexpr uint32_t G2_RED_T = 256;                // chunks (= threads of the per-window scan block) per window: four waves, one per SIMD
constexpr uint32_t G2_SEG_MIN = 4;                // fewest sorted entries per accumulate lane while the chip is not full
constexpr uint32_t G2_ACC_WAVES = 2;              // resident waves per SIMD of k_g2_accumulate (its register budget: g2msm.hip)
constexpr uint32_t G2_NP_SERIAL = 8;              // partials of one bucket above which a whole wave sums it (k_g2_bucket_fin)
constexpr uint32_t G2_WIRE_WORDS = 64;            // u32 of one wire XYZZ value (8 Fq)

// the workspace buffers of one launch, in the order the driver reserves them (the sort's own are those of `sort`)
enum G2WsBuffer { G2WS_HEAD, G2WS_CONT, G2WS_BUCKET, G2WS_CHUNK_S, G2WS_CHUNK_TMP, G2WS_CHUNK_A, G2WS_BUFFERS };

constexpr uint32_t G2_RESULT_CAP = MSM_MAX_OUT * 32 / G2_WIRE_WORDS;   // wire XYZZ values the pinned result buffer holds (8 192)
constexpr size_t G2_MAX_ENTRIES = (size_t)1 << 27;                     // sorted entries of one launch: the bound G2MSM_MAX_LAUNCH was chosen for
constexpr uint32_t G2_LANES_PER_BUCKET = 4;                            // nl <= 4 G: ~5 partials per bucket or fewer with uniform scalars (<= G2_NP_SERIAL)

// One launch: `blobs` scalar sets of n scalars each, every one against the same nb base sets of n points.  The blobs of a launch are ONE
// bucket problem: blobs * W bucket sets in one sort, one accumulate, one bucket pass and one reduction, with the base set as the second
// grid dimension.  A single MSM is the launch of one blob.
struct G2Plan {
    uint32_t n;          // scalars per blob
    uint32_t nb;         // base sets (1 or 2): grid.y of every kernel behind the sort
    uint32_t blobs;      // blobs of this launch
    int c, W;            // generic_window(n, 1), whatever blobs: never inflated to fit
    uint32_t B, G;       // buckets per window, blobs * W * B: the buckets of ONE base set
    uint32_t nl;         // accumulate lanes per base set (a multiple of 256)
    uint32_t seg;        // sorted entries per lane at most: ceil(blobs W n / nl) -- the kernel's ceil(E / nl) for its E <= blobs W n
    uint32_t T, m;       // reduction: chunks per window, buckets per chunk
    uint32_t n_out;      // wire XYZZ values left for the host: nb * blobs * W, value (s * blobs + b) * W + w
    uint32_t launches;   // kernel launches and memsets enqueued: the sort's and 6, whatever blobs and nb
    Plan sort;           // the generic-mode G1 plan of (n, c) with batch = blobs, marked shared_bases: digits, histogram, scan, scatter
    size_t bytes[G2WS_BUFFERS];
    size_t workspace_bytes;      // all device buffers of the launch, the sort's included

    uint32_t n_windows() const { return blobs * (uint32_t)W; }
    size_t entries() const { return (size_t)n_windows() * n; }
    uint32_t n_chunks() const { return n_windows() * T; }
    // most additions one lane of the bucket kernel performs: a bucket of up to G2_NP_SERIAL partials alone, heavier ones by the 64
    // lanes of its wave (strided partials, then a six-step tree) -- at most every lane's partial of the launch in one bucket
    uint32_t fin_adds_bound() const { return std::max<uint32_t>(G2_NP_SERIAL, (nl + 1 + 63) / 64 + 6); }
};

// Blobs per launch of a call of `count` blobs (the last launch may hold fewer), or 0: n = 0, a bad nb, or a blob above one launch (the
// driver takes such blobs in parts).  The largest group that keeps (1) the results inside the pinned buffer, (2) the sorted entries within
// G2_MAX_ENTRIES and (3) the bucket counts within the two-level scan -- one blob where no two fit; then max_blobs (0: no cap of the
// caller's) and the count.
inline uint32_t g2_batch_group(size_t n, uint32_t nb, size_t count, uint32_t max_blobs) {
    if (n == 0 || n > G2MSM_MAX_LAUNCH || nb < 1 || nb > 2) return 0;
    const int c = generic_window(n, 1);
    const size_t W = (size_t)(255 + c - 1) / c, B = (size_t)1 << (c - 1);
    size_t cap = G2_RESULT_CAP / (nb * W);
    cap = std::min(cap, G2_MAX_ENTRIES / (W * n));
    cap = std::min(cap, (size_t)SCAN_TILE * SCAN_TILE / (W * B));       // (G <= SCAN1_MAX < SCAN_TILE^2 is the smaller demand)
    cap = std::max<size_t>(cap, 1);
    if (max_blobs) cap = std::min<size_t>(cap, max_blobs);
    return (uint32_t)std::min(cap, std::max<size_t>(count, 1));
}
// whether a call of several blobs shares launches at all: one blob is at most one launch and a group of two fits
inline bool g2_batch_shares(size_t n, uint32_t nb) { return g2_batch_group(n, nb, 2, 0) == 2; }

// wave_slots: waves of the accumulate kernel the device holds at once (CUs * 4 SIMDs * G2_ACC_WAVES).  Total: g2_plan_status judges
// the result.
inline G2Plan g2_make_plan(size_t n, uint32_t nb, uint32_t blobs, uint32_t wave_slots) {
    G2Plan p{};
    p.n = (uint32_t)std::min<size_t>(n, 0xFFFFFFFFu);
    p.nb = nb;
    p.blobs = blobs;
    // window bits: generic_window(n, 1) as for G1 bases given by the caller.  A G2 addition costs ~2.8 G1 additions in BOTH the
    // accumulation (W n mixed additions) and the reduction (2 B W full additions), so the optimum of the ratio stays where it is.
    p.c = generic_window(std::max<size_t>(n, 1), 1);
    p.W = (255 + p.c - 1) / p.c;
    p.B = 1u << (p.c - 1);
    p.G = (uint32_t)std::min<size_t>((size_t)blobs * p.W * p.B, 0xFFFFFFFFu);
    PlanContext pc;
    pc.msm_c_override = p.c;
    p.sort = make_plan(pc, p.n, MsmBasesShape{}, std::max<uint32_t>(blobs, 1));
    p.sort.shared_bases = true;
    const size_t E = p.entries();
    // Lanes: an equal share of the sorted entries each, whatever the scalars -- one round of resident waves at most, G2_SEG_MIN entries
    // per lane at least, and no more than G2_LANES_PER_BUCKET lanes per bucket: a bucket's entries then spread over few lanes and
    // k_g2_bucket_fin sums it on its one-lane path
    size_t lanes = std::min<size_t>((size_t)std::max<uint32_t>(wave_slots, 4) * 64, (E + G2_SEG_MIN - 1) / G2_SEG_MIN);
    lanes = std::min<size_t>(lanes, (size_t)G2_LANES_PER_BUCKET * p.G);
    lanes = std::max<size_t>(256, (lanes + 255) / 256 * 256);
    p.nl = (uint32_t)lanes;
    p.seg = (uint32_t)((E + p.nl - 1) / p.nl);
    p.T = std::min<uint32_t>(p.B, G2_RED_T);
    p.m = p.B / p.T;
    p.n_out = (uint32_t)std::min<size_t>((size_t)nb * p.n_windows(), 0xFFFFFFFFu);
    const size_t point = (size_t)72 * 4;               // 72 limb planes
    p.bytes[G2WS_HEAD] = (size_t)nb * p.G * point;     // set s at s G of planes nb G apart
    p.bytes[G2WS_CONT] = (size_t)nb * p.nl * point;    // set s at s nl
    p.bytes[G2WS_BUCKET] = (size_t)nb * p.G * point;
    p.bytes[G2WS_CHUNK_S] = p.bytes[G2WS_CHUNK_TMP] = p.bytes[G2WS_CHUNK_A] = (size_t)nb * p.n_chunks() * point;     // set s at s n_chunks
    p.workspace_bytes = 0;
    for (int i = 0; i < G2WS_BUFFERS; ++i) p.workspace_bytes += p.bytes[i];
    for (int i = 0; i < WS_BUFFERS; ++i)
        if (i == WS_DIGITS || i == WS_SORTED || i == WS_COUNT || i == WS_BLOCKBASE || i == WS_OFFS || i == WS_BLOCK_SUMS) p.workspace_bytes += p.sort.bytes[i];
    // sort: counter memset, digits, (cursor memset,) histogram, scan (1 or 3), scatter; then accumulate, bucket sums and four reduction
    // kernels ONCE: the base set is their grid.y
    p.launches = 2 + (p.sort.sort_small ? 1u : 0u) + 1 + (p.sort.G <= SCAN1_MAX ? 1u : 3u) + 1 + 6;
    return p;
}

// KZG_OK, or the status the driver returns instead of launching.  out_cap: wire XYZZ values the result buffer holds.
inline int32_t g2_plan_status(const G2Plan& p, size_t n, uint32_t out_cap, const char** error) {
    *error = nullptr;
    if (n == 0 || p.blobs == 0 || (p.nb != 1 && p.nb != 2)) return KZG_ERR_INVALID_ARG;
    if (n > G2MSM_MAX_LAUNCH) { *error = "G2 MSM launch above G2MSM_MAX_LAUNCH scalars per blob (the driver splits longer MSMs)"; return KZG_ERR_INVALID_ARG; }
    if ((size_t)p.blobs * p.W * n > G2_MAX_ENTRIES) { *error = "G2 MSM: the launch's entries exceed G2_MAX_ENTRIES"; return KZG_ERR_INVALID_ARG; }
    if (!p.sort.shared_bases || p.sort.tables || p.sort.batch != p.blobs || p.sort.c != p.c || p.sort.W != p.W || p.sort.G != p.G) {
        *error = "G2 MSM: the sort's plan differs from the window plan";
        return KZG_ERR_INVALID_ARG;
    }
    if (p.G > SCAN1_MAX && p.sort.scan_blocks() > (uint32_t)SCAN_TILE) return KZG_ERR_INVALID_ARG;
    if (p.nl % 256 != 0 || (size_t)p.seg * p.nl < p.entries() || p.T * p.m != p.B || p.T > G2_RED_T) return KZG_ERR_INVALID_ARG;
    if ((size_t)p.nb * p.n_windows() > out_cap) { *error = "G2 MSM: the launch's result points exceed the result buffer"; return KZG_ERR_INVALID_ARG; }
    return KZG_OK;
}

}  // namespace kzg
