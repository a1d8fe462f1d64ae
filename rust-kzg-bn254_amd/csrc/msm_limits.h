// msm_limits.h — the sizes that the MSM kernels (msm_kernels.h) and the host planner (msm_plan.h) must agree on.  No device code and no
// HIP type: plain C++.  Each constant is explained where it is used; the section numbers are those of msm_kernels.h.
#pragma once
#include <cstddef>
#include <cstdint>

namespace kzg {

constexpr int RED_T = 512;          // chunks (= threads of the per-window scan block) per window

// 2. exclusive scan of the bucket counts
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;
constexpr int SCAN1_THREADS = 1024;             // the one-workgroup scan (k_scan_counts_1wg) ...
constexpr uint32_t SCAN1_MAX = 1u << 17;        // ... of up to this many counters

// 3b. two-level sort
constexpr int SORT2_LO_BITS = 7;
constexpr uint32_t SORT2_LO = 1u << SORT2_LO_BITS;
constexpr int SORT2_IDX_BITS = 24;
constexpr uint32_t SORT2_IDX_MASK = (1u << SORT2_IDX_BITS) - 1u;
constexpr uint32_t SORT2_CHUNK = 4096;          // entries per pass-2 tile of a LARGE bin
constexpr uint32_t SORT2_MAX_BINS = 512;
constexpr int SORT2_P1_THREADS = 512;
constexpr uint32_t SORT2_BIN_CAP = 65536;
constexpr int SORT2_BIN_THREADS = 1024;
constexpr int SORT2_BIN_PER = 8;                                        // entries per thread and chunk
constexpr uint32_t SORT2_BIN_CHUNK = SORT2_BIN_THREADS * SORT2_BIN_PER;
constexpr size_t SORT1_MAX_LDS = 131072;       // single-pass sort: one LDS counter per bucket (<= 2^15 buckets)

constexpr int MSM_BATCH_PTRS = 16;              // separate scalar buffers of one batched launch (PolyPtrs)
constexpr uint32_t BITSUM_MAX_N = 8192;     // what the kernels take; the default policy (engine.h srs_bases) uses them up to 4 096

constexpr uint32_t MSM_BATCH_POLYS_MAX = 1024;  // polynomials of one batched table-mode launch (64 buckets each: 2^16 buckets)
constexpr uint32_t MSM_MAX_OUT = 16384;        // XYZZ values one launch may hand to the host epilogue (generic mode: W * batch window sums)
// Largest number of pairs one launch takes: W * n must fit the 32-bit positions of the sort.
static const size_t MSM_MAX_LAUNCH = (size_t)1 << 24;
// One asynchronous MSM = up to MSM_MAX_PARTS launches back to back on the slot's stream, sharing its workspace (stream order keeps
// them apart); each copies its O(200) result points to its own MSM_PART_OUT-point window of the pinned buffer.
constexpr uint32_t MSM_MAX_PARTS = 64;       // round 4: 64 launches (2^26 pairs over a table-mode SRS of more than 2^20 points); 16 before
constexpr uint32_t MSM_PART_OUT = MSM_MAX_OUT / MSM_MAX_PARTS;

}  // namespace kzg
