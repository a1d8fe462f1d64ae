// engine.h — host-side objects behind the C-ABI (include/kzg_bn254_mi355x.h): one context per GPU,
// device-resident SRS, reusable workspaces.  No torch types, no CPU fallback.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include "../../include/kzg_bn254_mi355x.h"
#include "msm_plan.h"      // MsmBasesShape, msm_batch_capacity
#include "host_recover.h"  // RecoverPlan, RecoverBatchPlan
#include "host_encode.h"   // EncodePlan
#include "host_locate.h"   // LocatePlan
#include "host_prove_cosets.h"   // ProveCosetsPlan
#include "host_prove_batch.h"    // ProveBatchPlan, the group budget
#include "host_coset_mixed.h"    // MixedPlan

namespace kzg_host { struct G1; struct G2; }   // host_pairing.h
namespace kzg {

struct DeviceBuffer {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t reserve(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; bytes = 0; if (e != hipSuccess) return e; }
        size_t cap = need + need / 8;
        hipError_t e = hipMalloc(&p, cap);
        if (e == hipSuccess) bytes = cap;
        return e;
    }
    void release() { if (p) { (void)hipFree(p); p = nullptr; bytes = 0; } }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct MsmWorkspace {
    DeviceBuffer scalars;      // staging for host scalars (n x 32 B)
    DeviceBuffer blob;         // staging for blob bytes (asynchronous commit_blob)
    DeviceBuffer bases;        // staging for ad-hoc bases (n x 64 B, device format)
    DeviceBuffer bases_wire;   // staging for ad-hoc bases in wire format
    DeviceBuffer digits, sorted, count, blockbase, sort_tmp, sort_key, sort_small, offs, block_sums, bucket, chunkS, chunkTmp, chunkA, out_wire;
    DeviceBuffer head, cont;   // accumulate partials: head[g] per bucket, cont[t] per lane (36 limb planes each; msm_kernels.h section 4)
    const void* count_zero_ptr = nullptr;   // `count` at this address holds zeros in its first count_zero_g words once the stream gets here (small table-mode sort: the scan clears what it read)
    uint32_t count_zero_g = 0;
    void* pinned_out = nullptr;   // pinned host buffer for window sums
    void* pinned_out_dev = nullptr;   // its device address: the reduction kernels store their results there directly
    // optional per-phase timing with HIP events on the launch stream (kzg_ctx_set_profiling)
    static constexpr int N_PHASES = 8;   // digits, sort (histograms + scan), scatter, (unused), accumulate, bucket sums + reduce level 1, reduce level 2, whole launch
    hipEvent_t ev[N_PHASES] = {};
    bool ev_ready = false;
    hipEvent_t ev_done = nullptr;   // recorded behind the result copy of the MSM in flight on this workspace
    hipEvent_t ev_sorted = nullptr; // recorded behind the sort of that MSM (in front of its accumulate kernel): the next MSM of the context starts behind it
    double phase_ms[N_PHASES] = {};
    uint64_t profiled_launches = 0;
    uint64_t profiled_pairs = 0;
    uint64_t profiled_entries = 0;   // sorted entries (= mixed additions) of the profiled launches
    void release();
};

// scratch of the polynomial kernels: a = evaluations / bytes->Fr output, b = inverses | denominators (limb planes),
// c = quotient / blob bytes, small = scalars and per-block partial sums; pinned = 4 KiB host staging (init image, z, y readback)
struct PolySet {
    DeviceBuffer a, b, c, small;
    void* pinned = nullptr;
    hipEvent_t ev_chain = nullptr;   // behind the inversion chain of a proof when it runs on the auxiliary stream (poly.hip proof_enqueue)
    void release() {
        a.release(); b.release(); c.release(); small.release();
        if (pinned) { (void)hipHostFree(pinned); pinned = nullptr; }
        if (ev_chain) { (void)hipEventDestroy(ev_chain); ev_chain = nullptr; }
    }
};

struct NttWorkspace {
    DeviceBuffer data, tmp;
    void release() { data.release(); tmp.release(); }
};

}  // namespace kzg

namespace kzg {
struct MsmPending;
struct BlobStream;   // blob -> commitment + proof jobs in flight (blobstream.hip)
// a proof over a slice of the evaluations and the matching slice of a Lagrange basis, in flight on one slot (lagrange.hip)
struct LagProof {
    int phase = 0;                 // 0 idle; 1 inverses + partial barycentric sum enqueued; 2 partial collected, waiting for y; 3 quotient (+ MSM) enqueued
    const kzg_srs* shard = nullptr;
    const void* d_evals = nullptr; // the caller's resident evaluations (read in place), or nullptr: the slot's copy
    size_t base = 0, len = 0, n = 0;   // the slice holds the evaluations [base, base + len) of the n-point domain
    bool on_domain = false;        // z = w^m
    uint32_t m = 0;
    bool msm_started = false;      // len > 0: an MSM is pending on the slot
    bool grouped = false;          // commitment and proof leave as ONE batched launch (two scalar sets) on this slot
    bool owns_m() const { return on_domain && m >= base && m - base < len; }   // z = w^m and this slice holds f_m
};
}
#ifndef KZG_NUM_SLOTS
#define KZG_NUM_SLOTS 4      // slots of the asynchronous calls (include/kzg_bn254_mi355x.h: KZG_NUM_SLOTS)
#endif

struct kzg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::string last_error;
    int msm_c_override = 0;
    int msm_seg_override = 0;
    size_t encode_group_bytes = 0;         // kzg_ctx_set_encode_group_bytes: the workspace budget of a group of kzg_encode_cosets_batch, 0 = ENCODE_GROUP_BYTES_DEFAULT
    size_t recover_group_bytes = 0;        // kzg_ctx_set_recover_group_bytes: the same for kzg_recover_from_cosets_batch, 0 = RECOVER_GROUP_BYTES_DEFAULT
    uint32_t g2_batch_group = 0;           // kzg_ctx_set_g2_batch_group: most blobs per group of the batched G2 MSM, 0 = the planner's choice (g2msm_plan.h)
    int reduction_lanes = 0;               // kzg_ctx_set_reduction_lanes: 0 automatic, 2 lane pairs, 4 lane quads
    std::atomic<int> transcript_device{0}; // kzg_ctx_set_transcript_device: 0 automatic, 1 always host, 2 always device (the weights of kzg_verify_multiproof_batch)
    bool profiling = false;
    bool lds_attr_set = false;
    bool poly_lds_attr_set = false;
    uint32_t acc_wave_slots = 3 * 1024;   // resident waves of the accumulate kernel on this device: 3 per SIMD x 4 SIMDs x CUs (set at kzg_ctx_create; msm_plan.h make_plan takes 2 of the 3 per SIMD where that pays)
    kzg::MsmWorkspace msm;
    kzg::MsmWorkspace msm_x[KZG_NUM_SLOTS - 1];   // workspaces of slots 1.. of the asynchronous calls
    hipStream_t stream_x[KZG_NUM_SLOTS - 1] = {}; // one stream per slot (slot 0: `stream`), created on first use
    kzg::MsmPending* slot_pending[KZG_NUM_SLOTS] = {};   // what each slot of the asynchronous calls has in flight
    kzg::NttWorkspace ntt;
    int32_t* ondomain_inv[13] = {};      // [log n] -> 1 / (w^k - 1), k < n <= 4096 (limb planes): proofs at a known domain point (poly.hip)
    kzg::NttWorkspace ntt_x[KZG_NUM_SLOTS - 1];   // slots 1.. of the asynchronous commitment / proof calls
    void* vb_pinned = nullptr;           // pinned staging of the packed blobs of one batch verification (capi_verify.hip), grown on demand
    size_t vb_pinned_bytes = 0;
    kzg::DeviceBuffer rccl_buf;          // this rank's partial + the gathered partials of kzg_rccl_allgather_fold (multi.hip)
    void* rccl_pinned = nullptr;         // pinned host staging of the same rows (row out | world rows in)
    size_t rccl_pinned_bytes = 0;
    kzg::PolySet poly[KZG_NUM_SLOTS];   // polynomial / proof pipeline scratch, one set per slot ([0] also serves the synchronous calls)
    kzg::LagProof lag[KZG_NUM_SLOTS];   // Lagrange-sharded proofs in flight (kzg_compute_proof_lagrange_*)
    hipStream_t lag_stream = nullptr;       // high-priority stream of phase 1 (upload, inverses, partial sum) of every Lagrange-sharded proof of this context
    hipEvent_t lag_phase1[KZG_NUM_SLOTS] = {};     // behind phase 1 of the proof on that slot
    hipEvent_t lag_uploaded[KZG_NUM_SLOTS] = {};   // behind the slice's upload on the proof slot's stream: the commitment on another slot starts after it
    kzg::MsmWorkspace& slot_msm(int slot) { return slot ? msm_x[slot - 1] : msm; }
    kzg::BlobStream* blob_stream = nullptr;    // kzg_commit_and_prove_blob_begin / _end: created on first use
    hipEvent_t last_sorted = nullptr;          // ev_sorted of the most recently enqueued MSM launch of this context ...
    hipStream_t last_sorted_stream = nullptr;  // ... and the stream it went to (msm.hip enqueue_sort)
    kzg::NttWorkspace& slot_ntt(int slot) { return slot ? ntt_x[slot - 1] : ntt; }
    kzg::DeviceBuffer mp[6];                   // scratch of kzg_compute_multiproofs / kzg_srs_cache_multiproof (multiproof.hip), its own: slot 0's may be in flight
    kzg::NttWorkspace mp_ntt;
    kzg::DeviceBuffer mv[4];                   // kzg_coset_interpolate_rlc / kzg_verify_multiproof_batch (multiverify.hip): values | indices + weights | coefficients | partial rows
    kzg::NttWorkspace mv_ntt;
    kzg::DeviceBuffer ml[6];                   // kzg_coset_group_sums / kzg_verify_multiproof_batch_locate (multilocate.hip): group coefficients | the plan's arrays | partial point sums | group sums | rows + shifted weights | proofs + commitments; kzg_header_group_sums (capi_g2.hip) works in [1] .. [5] the same way
    kzg::DeviceBuffer fs[2];                  // the coset transcript on the device (fsdevice.hip): commitment rows | proofs, digests | power tables | flag; kzg_sha256_rows: messages, digests
    kzg::DeviceBuffer cb[2];                   // serialized coset items (cosetbytes.hip): value bytes | point bytes (commitments, proofs), decoded wire points, the bad words
    kzg::DeviceBuffer rc[3];                   // kzg_recover_from_cosets(_batch) (recover.hip), for a group of blobs: work values | item maps, patterns, missing lists, flags, vanishing values, partial products (RecoverBatchPlan's layout), then the bad word of a call on serialized values | powers of g
    int rc_gpow_log = -1;                      // rc[2] holds the factored tables of g^t and g^-t for t < 2^rc_gpow_log (-1: none yet)
    kzg::NttWorkspace rc_ntt;                  // its `data` also stages the uploaded coset values (dead before the first transform) and the compacted rows of out_len < n (after the last)
    kzg::DeviceBuffer pc[4];                   // kzg_prove_cosets / kzg_coset_quotients (provecosets.hip): the referenced polynomials' coefficients | a group's quotient rows | its heads block, then its twisted remainders | its items' polynomial slots and coset indices
    kzg::NttWorkspace pc_ntt;                  // the inverse transforms of eval-form polynomials, the l-point transforms of the values
    kzg::DeviceBuffer pr[4];                   // batched pairing checks (pairing.hip; host_pairing_batch.h PairingBatchPlan): wire points | device-format points, offsets, flags | GT words, verdicts | the constants of the device pairing
    bool pr_consts_ready = false;              // pr[3] holds them (uploaded at the context's first batch)
    kzg::DeviceBuffer pb[4];                   // the batched prover (provebatch.hip), for a group of one length class: packed blob bytes, descriptors | rows of evaluations | quotient rows | zs, ys, prep records
    size_t prove_group_bytes = 0;              // kzg_ctx_set_prove_group_bytes: the workspace budget of such a group, 0 = PROVE_GROUP_BYTES_DEFAULT (host_prove_batch.h)
    std::atomic<int> locate_pairings{0};       // kzg_ctx_set_locate_pairings: 0 = the located coset verifiers search on the host, 1 = they evaluate every group's equation on the device
};

struct kzg_srs {
    kzg_ctx* ctx = nullptr;
    // An SRS may be used by several host threads and by every context of its GPU at once (the reference shares one SRS across threads:
    // prover/tests/kzg_test.rs:9-17).  Everything below that is built AFTER the handle was returned -- per-bit tables on the first batched
    // call, the x3 tables of g1_ifft, cached Lagrange bases -- is built and published under lazy_mu, fully synchronised before the pointer
    // is stored, and read through the accessors below (a reader sees "absent" or "complete", never a table under construction).
    mutable std::mutex lazy_mu;
    // device affine format (curve.h), 64 B per point.  Without precomputation: n points.  With precomputed
    // window tables (pre_W > 0): pre_W x n points, table w holds T_w[i] = 2^(pre_c * w) * P_i (table 0 = the SRS).
    uint4* d_points = nullptr;
    size_t n = 0;
    int pre_c = 0;
    int pre_W = 0;
    // second table set with narrower windows (small_c < pre_c) for MSMs of at most SRS_SMALL_MAX pairs (srs.hip); may be absent
    uint4* d_small = nullptr;
    int small_c = 0;
    int small_W = 0;
    // per-bit tables Bit_j[i] = 2^j P_i, j < 255, n points apart (srs.hip srs_build_bit_tables): the NAF mode of MSMs of >= SRS_NAF_MIN pairs; may be absent
    uint4* d_bits = nullptr;
    // no point of this SRS is the identity (srs.hip srs_precompute counts them before it builds the tables; a doubled identity is the
    // identity, so the one flag covers every table): the accumulate kernel of its MSMs then runs without the per-entry identity test.
    // false = unknown or some: the test stays
    bool identity_free = false;
    // 3 Bit_p[j] for p < 255, j < 256 (g1fft.hip: the x3 tables of the 64..256-point g1_ifft), built on first use; a cache, hence mutable
    mutable uint4* d_t3 = nullptr;
    mutable uint32_t t3_n = 0;           // points covered by d_t3: min(n, 2048)
    // Lagrange-basis copies of the first m points (KZG::g1_ifft(m), kzg.rs:263-285), built by kzg_srs_cache_lagrange and used by
    // the eval-form commitments of exactly m evaluations instead of IFFT + MSM over the monomial basis; owned by this SRS
    std::map<size_t, kzg_srs*> lagrange;
    size_t lagrange_of = 0;      // this handle IS a Lagrange basis of that many points (0: monomial SRS)
    // FK20 multi-proofs (multiproof.hip): (n, chunk length l) -> FFT_2m(S^(b)) for b < l, m = n / l, as l x 2m affine points (device format,
    // 2n points), built by kzg_srs_cache_multiproof or on first use and published under lazy_mu like `lagrange`; owned by this SRS
    std::map<std::pair<size_t, size_t>, uint4*> multiproof;
};

// A device-resident G2 SRS: n affine points on the twist in the device format of curve_g2.h, 128 B per point, no tables
struct kzg_g2srs {
    kzg_ctx* ctx = nullptr;
    uint4* d_points = nullptr;
    size_t n = 0;
};

namespace kzg {

// Bases of one MSM: `points` = first base of the slice; the shape (msm_plan.h) selects the mode.
struct MsmBases : MsmBasesShape {
    const uint4* points = nullptr;
    bool identity_free = false;   // known: none of the points (of any table) is the identity (kzg_srs::identity_free; caller bases: unknown)
};
constexpr int SRS_SMALL_C = 15;                       // window bits of the second table set
constexpr size_t SRS_SMALL_MAX = (size_t)1 << 13;     // MSMs of up to this many pairs use it
constexpr size_t SRS_NAF_MIN = (size_t)1 << 11;       // an SRS of at least this many points gets per-bit tables at upload (16 KiB per point; from 2^15 points for the NAF mode of large MSMs, below for the bit sums of tiny ones)
constexpr size_t MSM_NAF_MIN = (size_t)1 << 14;       // MSMs of at least this many pairs use them (width-w NAF digits): one at a time 2^14 0.296 -> 0.273 ms; 2^13 0.241 -> 0.273: not below
// bucket bits (c: 2^(c-1) buckets, NAF width c + 1) of an MSM of n pairs over the per-bit tables: the window policy of srs_precompute, by MSM length
inline int srs_naf_c(size_t n) {
    if (n < ((size_t)1 << 15)) return 13;                                       // (13: 32 digit words per scalar; 15..17: 16)
    // measured (tools/time_shard_inflight.py, c = 15 / 16 / 17, two or three MSMs in flight, ms per MSM): 2^17 0.257 / 0.264 / 0.284,
    // 2^18 0.362 / 0.355 / 0.404, 2^19 0.678 / 0.631 / 0.629, 2^20 1.307 / 1.227 / 1.188 (profiles/r03_naf.md)
    return n >= ((size_t)1 << 20) ? 17 : n >= ((size_t)1 << 18) ? 16 : 15;
}
// bases of an MSM of n pairs over srs[offset .. offset + n)
inline uint4* srs_bits(const kzg_srs* srs) { std::lock_guard<std::mutex> lk(srs->lazy_mu); return srs->d_bits; }
inline uint4* srs_t3(const kzg_srs* srs) { std::lock_guard<std::mutex> lk(srs->lazy_mu); return srs->d_t3; }
inline kzg_srs* srs_cached_lagrange(const kzg_srs* srs, size_t n) {
    std::lock_guard<std::mutex> lk(srs->lazy_mu);
    auto it = srs->lagrange.find(n);
    return it == srs->lagrange.end() ? nullptr : it->second;
}
inline MsmBases srs_bases(const kzg_srs* srs, size_t offset, size_t n, bool allow_tables) {
    MsmBases b;
    std::lock_guard<std::mutex> lk(srs->lazy_mu);
    b.points = srs->d_points + 4 * offset;
    b.identity_free = srs->identity_free;
    if (allow_tables && srs->pre_W > 0) {
        b.table_stride = (uint32_t)srs->n; b.c = srs->pre_c; b.W = srs->pre_W;
        if (srs->d_small && n <= SRS_SMALL_MAX) { b.points = srs->d_small + 4 * offset; b.c = srs->small_c; b.W = srs->small_W; }
        // bit sums up to 4 096 pairs; measured, one commitment at a time: 2^9 0.108 -> 0.066 ms, 2^10 0.120 -> 0.077, 2^11 0.157 -> 0.100, 2^12 0.176 -> 0.135, 2^13 0.197 -> 0.204
        if (srs->d_bits && n <= 4096) {
            b.points = srs->d_bits + 4 * offset; b.c = 0; b.W = 255; b.bitsum = true;
        }
        if (srs->d_bits && n >= MSM_NAF_MIN) {
            b.points = srs->d_bits + 4 * offset; b.c = srs_naf_c(n); b.W = 255; b.naf = true;
        }
    }
    return b;
}

// MSM over device-resident points (device format) and device-resident scalars (wire format).
// Writes the affine result (or the XYZZ partial if out_xyzz != nullptr).
int32_t msm_run(kzg_ctx* ctx, const MsmBases& bases, const void* d_scalars, size_t n,
                uint64_t out_xy[8], uint8_t* out_inf, uint64_t* out_xyzz);

int32_t msm_slot_stream(kzg_ctx* ctx, int slot, hipStream_t* out);
int32_t msm_begin(kzg_ctx* ctx, int slot, const MsmBases& bases, const void* d_scalars, size_t n);
int32_t msm_end(kzg_ctx* ctx, int slot, uint64_t out_xy[8], uint8_t* out_inf, uint64_t* out_xyzz);
void msm_drop_slots(kzg_ctx* ctx);
// the pieces of the G1 driver the G2 driver (g2msm.hip) runs on: the pinned result buffer of a workspace, and the digits + counting sort of
// one generic-mode scalar set (p: make_plan without tables, batch 1), which leave ws.sorted / ws.offs
int32_t msm_pinned_out(kzg_ctx* ctx, MsmWorkspace& ws);
int32_t msm_sort_generic(kzg_ctx* ctx, MsmWorkspace& ws, hipStream_t st, const uint4* d_scalars, const Plan& p);
int32_t msm_run_batch(kzg_ctx* ctx, const uint4* d_points, const void* d_scalars, size_t n, uint32_t batch,
                      uint64_t* out_xy, uint8_t* out_inf);

// Precompute the window tables of an SRS in place (reallocates srs->d_points); no-op for small / huge SRS.
int32_t srs_precompute(kzg_ctx* ctx, kzg_srs* srs);
int32_t srs_build_bit_tables(kzg_ctx* ctx, kzg_srs* srs, bool force);
// `polys` commitments over the first n points of one SRS in one kernel sequence (bases: the SRS's per-bit tables; msm.hip)
int32_t msm_begin_batch(kzg_ctx* ctx, int slot, const MsmBases& bases, const void* const* d_scalars, size_t n, size_t count);
int32_t msm_end_batch(kzg_ctx* ctx, int slot, size_t count, uint64_t* out_xy, uint8_t* out_inf, uint64_t* out_xyzz);
int32_t msm_run_batch_tables(kzg_ctx* ctx, const MsmBases& bases, const void* d_scalars, size_t n, size_t polys, uint64_t* out_xy, uint8_t* out_inf);

// wire affine points (device memory) -> device affine format (curve.h), asynchronous on ctx->stream
// d_off_curve_flag != nullptr: also check y^2 == x^3 + 3 of every non-identity point, *flag |= 1 on a violation (device word, zeroed by the caller)
int32_t points_wire_to_device(kzg_ctx* ctx, const uint4* d_wire, uint4* d_out, size_t n, uint32_t* d_off_curve_flag = nullptr);

// Two-level twiddle table of one domain: w^t (t < lo_len) and w^(t * lo_len) (t < hi_len), 9 limb planes each,
// internal Montgomery form.  Cached per (device, log n, direction).
struct NttTables {
    int32_t* lo = nullptr;
    int32_t* hi = nullptr;
    uint32_t lo_len = 0, hi_len = 0;
    int lo_bits = 0;
};
int32_t ntt_get_tables(kzg_ctx* ctx, int log_n, bool inverse, NttTables* out);

// In-place NTT on device data (wire format), natural order in/out.
int32_t ntt_run(kzg_ctx* ctx, void* d_data, size_t n, bool inverse, hipStream_t st = nullptr, NttWorkspace* ws = nullptr);
// `rows` transforms of n points, row r at d_data + r n elements, one launch per pass (ntt_run is rows = 1)
int32_t ntt_run_batch(kzg_ctx* ctx, void* d_data, size_t n, size_t rows, bool inverse, hipStream_t st = nullptr, NttWorkspace* ws = nullptr);

// synthetic SRS P_i = tau^i * G1 written to d_points (device format); device SRS -> wire on the host
int32_t srs_generate(kzg_ctx* ctx, const uint64_t tau_mont[4], uint64_t first_power, size_t n, uint4* d_points);
int32_t srs_download(kzg_ctx* ctx, const uint4* d_points, size_t n, uint64_t* out_xy);
int32_t fr_powers_canonical(kzg_ctx* ctx, const uint64_t tau_mont[4], uint64_t first_power, size_t n, const uint4** d_out);

// G2 (g2msm.hip).  Called under ctx->mu with the device set; every one is synchronised on return.
// the MSM of ONE scalar set (device, wire form) over nb <= 2 base sets (device format, 8 uint4 per point): g2_msm_batch_run with count = 1;
// out: nb x 16 u64 affine wire points, out_inf: nb flags (may be null)
int32_t g2_msm_run(kzg_ctx* ctx, const uint4* const* d_points, uint32_t nb, const void* d_scalars, size_t n, uint64_t* out_g2, uint8_t* out_inf);
// `count` scalar sets of n scalars each (device, wire form, one after the other), ALL over the same nb <= 2 base sets of n points: groups of
// blobs planned by g2_batch_group (g2msm_plan.h; ctx->g2_batch_group caps them), one sort and one launch sequence per group for every
// blob and base set in it; a blob above G2MSM_MAX_LAUNCH scalars alone, in parts.  out_g2[s]: count x 16 u64 affine wire points of base set s, out_inf[s]: count flags (the array or an entry may be null)
int32_t g2_msm_batch_run(kzg_ctx* ctx, const uint4* const* d_points, uint32_t nb, const void* d_scalars, size_t n, size_t count, uint64_t* const* out_g2,
                         uint8_t* const* out_inf);
// n wire points of the host -> device format at d_out, every point checked on the twist (or the identity); *bad = index of the first one off it, or -1
int32_t g2_upload_points(kzg_ctx* ctx, const uint64_t* g2_mont, size_t n, uint4* d_out, int64_t* bad);
int32_t g2_generate_points(kzg_ctx* ctx, const uint64_t tau_mont[4], uint64_t first_power, size_t n, uint4* d_out);
int32_t g2_download_points(kzg_ctx* ctx, const uint4* d_points, size_t n, uint64_t* out_g2_mont);
// g2batch.hip: per-lane G2 chains over device-format points (g2_chain.h).  *bad = the smallest index of a point that is neither the identity nor in
// the order-r subgroup, or -1 (the points are on the twist: g2_upload_points checks that)
int32_t g2_subgroup_check(kzg_ctx* ctx, const uint4* d_points, size_t n, int64_t* bad);
// Lane t multiplies point lanes[t] (0xFFFFFFFF: an idle lane) by weight lanes[t] >> weight_shift (8 canonical u32 words each, the low `bits` bits read) and
// every tile of 64 lanes is summed: out_tiles_g2 = n_lanes / 64 affine wire points.  n_lanes is a multiple of 64.
int32_t g2_weighted_tile_sums(kzg_ctx* ctx, const uint4* d_points, size_t n_points, const uint32_t* lanes, size_t n_lanes, const uint32_t* weights_canonical,
                              size_t n_weights, uint32_t weight_shift, int bits, uint64_t* out_tiles_g2);
// One sum per SEGMENT of a plan over one key per point (locate_plan of host_locate.h on n_points keys): point p is multiplied by weight p >> 1 (canonical
// words, the low `bits` bits) and the points of a segment are summed: out_seg_g2 = plan.segs.size() affine wire points.  n_points <= 2^21.  Uses ctx->ml[1..3]
int32_t g2_locate_segment_sums(kzg_ctx* ctx, const uint4* d_points, size_t n_points, const LocatePlan& plan, const uint32_t* weights_canonical, size_t n_weights,
                               int bits, uint64_t* out_seg_g2);
// g2decode.hip: n gnark-compressed points of the host decoded on the device (g2_decode.h; flags: KZG_G2_CHECK_SUBGROUP | KZG_G2_REJECT_GENERATOR) into
// d_points (device format) or, with d_points == nullptr, as wire points to out_wire (host; written only when no point is refused).  Called under
// ctx->mu with slot 0 idle: the bytes go up through a ByteStager (byte_stager.h).  Synchronised on return.
// *bad_word = index << 2 | kind (G2_BAD_* of g2_decode.h) of the smallest refused index, or 0xFFFFFFFF
int32_t g2_decompress_run(kzg_ctx* ctx, const uint8_t* bytes, size_t n, uint32_t flags, uint4* d_points, uint64_t* out_wire, uint32_t* bad_word);
// the status of such a bad word (KZG_OK for 0xFFFFFFFF), its index to *bad_index (may be null), a line for kzg_ctx_last_error
int32_t g2_decode_status(kzg_ctx* ctx, const char* who, uint32_t bad_word, uint64_t* bad_index);
int32_t srs_decompress(kzg_ctx* ctx, const uint8_t* bytes, size_t n, uint4* d_points, uint32_t* err_kind, uint32_t* err_index, bool ark_le = false);

// KZG::g1_ifft: Lagrange-basis SRS of size n (n a power of two <= srs->n), affine wire points to the host / left on the device
int32_t g1_ifft_run(kzg_ctx* ctx, const kzg_srs* srs, size_t n, uint64_t* out_xy);
int32_t g1_ifft_device(kzg_ctx* ctx, const kzg_srs* srs, size_t n, uint4* d_out, bool wire);
// the generic G1 transform of XYZZ planes (g1fft.hip): forward or inverse, optional 1/n, input read with its own stride; and the
// batched affine conversion of n planes.  Both enqueued on st.
// a batch of transforms in one launch sequence: `batch` plane sets, in_batch / out_batch / tmp_batch words apart (the default: one transform)
struct G1fftBatch { size_t batch = 1, in_batch = 0, out_batch = 0, tmp_batch = 0; };
int32_t g1_fft_planes(kzg_ctx* ctx, hipStream_t st, const int32_t* in, size_t in_stride, size_t n, int32_t* out, int32_t* tmp, bool inverse, bool scaled, const G1fftBatch& b = G1fftBatch());
// the forward transform of an input that is the identity from point `nonzero` on (host_encode.h: the spread load of the radix-2 form)
int32_t g1_fft_planes_padded(kzg_ctx* ctx, hipStream_t st, const int32_t* in, size_t in_stride, size_t nonzero, size_t n, int32_t* out, int32_t* tmp, const G1fftBatch& b = G1fftBatch());
// compressed: 32 gnark-compressed bytes per point (g1_decode.h g1_compress_point; the identity is in the bytes) instead of 64
int32_t g1fft_planes_to_affine(kzg_ctx* ctx, hipStream_t st, const int32_t* planes, size_t n, uint4* d_out, bool wire, int32_t* scratch, size_t batch = 1, size_t planes_batch = 0,
                               bool compressed = false);
// FK20 multi-proofs (multiproof.hip): the cached FFT_2m(S^(b)) of (srs, n, l), built if absent; the proofs of every coset of l points
int32_t multiproof_cache(kzg_ctx* ctx, kzg_srs* srs, size_t n, size_t l, const uint4** out);
int32_t multiproof_run(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* poly_mont, size_t n, bool eval_form, size_t l, uint64_t* out_xy, uint8_t* out_inf);
void multiproof_drop(kzg_srs* srs);
// kzg_encode_cosets (multiproof.hip): the m = n / l cosets of values and their proofs for d = plan.d coefficients or evaluations;
// either output may be null.  Called under ctx->mu with the arguments checked, synchronised on return
int32_t multiproof_encode(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* poly_mont, bool eval_form, const EncodePlan& plan, uint64_t* out_ys, uint64_t* out_xy, uint8_t* out_inf);
// kzg_encode_cosets_batch: plan.count blobs of that shape, group by group (host_encode.h EncodeBatchPlan); row b of every output is that of multiproof_encode on blob b
int32_t multiproof_encode_batch(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* polys_mont, bool eval_form, const EncodeBatchPlan& plan, uint64_t* out_ys, uint64_t* out_xy, uint8_t* out_inf);
// The SERIALIZED form of the same driver (kzg_encode_cosets_batch_bytes, kzg_disperse_blobs_bytes): the blobs are 32-byte big-endian integers, decoded on the
// device where the group's first kernel loads them; values leave as 32 big-endian bytes each, proofs as 32 gnark-compressed bytes (no flag array).  Per group the
// decoded coefficients also feed commit_batch_device (commitments_be: 32 B per blob) and, with g2_points set, g2_msm_batch_run over the two base sets (64 B per
// blob each); those points are compressed on the host.  A value >= r ends the call at its group with KZG_ERR_DESERIALIZE and *bad_word = (the smallest bad
// b poly_len + i of that group) << 2, before any output of that group is written (needs count x poly_len <= 2^28).  Needs slot 0 idle when commitments_be is set.
struct EncodeBytesIo {
    const uint8_t* blobs_be = nullptr;          // count x d x 32
    uint8_t* ys_be = nullptr;                   // count x n x 32 or null (plan.values)
    uint8_t* proofs_be = nullptr;               // count x m x 32 or null (plan.proofs)
    uint8_t* commitments_be = nullptr;          // count x 32 or null
    const uint4* g2_points[2] = {nullptr, nullptr};   // the disperser's call: the G2 SRS and the trailing powers from their offset (device format), d points each
    uint8_t* length_commitments_be = nullptr;   // count x 64 each
    uint8_t* length_proofs_be = nullptr;
    uint32_t* bad_word = nullptr;               // may be null
};
int32_t multiproof_encode_batch_bytes(kzg_ctx* ctx, kzg_srs* srs, bool eval_form, const EncodeBatchPlan& plan, const EncodeBytesIo& io);
// verification of coset proofs (multiverify.hip): d_out[t] = sum_i weights[i] w^(-ks[i] t) IFFT_l(ys_i)[t], enqueued on ctx->stream (d_ys is scratch when l > 1024)
int32_t coset_interpolate_rlc_device(kzg_ctx* ctx, uint4* d_ys, const uint64_t* d_ks, const uint4* d_weights, size_t count, size_t n, size_t l, uint4* d_out);
// the same for items of mixed shapes (host_coset_mixed.h MixedPlan): d_out[t] = the sum over the items with l > t, t < l_max.  The plan's tables on the
// device: perm, val_off (u32 per item), the class of each workgroup of the two launches, MixedClassDev per class, MixedRow per row
struct MixedDevTables { const uint32_t *perm, *val_off, *wg_class[2]; const void *classes, *rows; };
int32_t coset_interpolate_rlc_mixed_device(kzg_ctx* ctx, const kzg_host::MixedPlan& p, uint4* d_ys, const uint64_t* d_ks, const uint4* d_weights,
                                           const MixedDevTables& t, uint4* d_out);
// locating the bad groups of a batch (multilocate.hip; LocatePlan: host_locate.h).  Called under ctx->mu with the device set, count > 0.
// the plan's arrays -> ctx->ml[1] (enqueued); the coefficients A_{g,t} of every non-empty group -> ctx->ml[0], d_ys overwritten (enqueued);
// per non-empty group the XYZZ wire words of sum r_i pi_i and sum (r_i C_{c_i} + r_i w^(k_i l) pi_i) -> out_xyzz, 2 x 16 u64 each (synchronised)
int32_t locate_upload_plan(kzg_ctx* ctx, const LocatePlan& plan);
int32_t coset_group_coeffs_device(kzg_ctx* ctx, uint4* d_ys, const uint64_t* d_ks, const uint4* d_weights, const LocatePlan& plan, size_t n, size_t l);
// its two halves, for a caller that sums the SAME items under more than one plan (kzg_retrieve_blobs_bytes_tolerant): the per-item rows
// r_i w^(-k_i t) IFFT_l(ys_i)_t over d_ys, which do not depend on the partition (transformed: l > 1024 and d_ys already holds IFFT_l(ys_i), as
// coset_interpolate_rlc_device leaves it), then the segment sums of a plan (which may cover a subset of the items) -> ctx->ml[0].  Enqueued.
int32_t coset_item_rows_device(kzg_ctx* ctx, uint4* d_ys, const uint64_t* d_ks, const uint4* d_weights, size_t count, size_t n, size_t l, bool transformed);
int32_t coset_seg_sums_device(kzg_ctx* ctx, const uint4* d_rows, const LocatePlan& plan, size_t l);
// n_proofs: the proofs in front of the commitments in d_points (0: plan.count, a plan over all items; a subset plan names items below n_proofs)
int32_t locate_point_sums_device(kzg_ctx* ctx, const uint4* d_points, const uint64_t* d_ci, const uint4* d_w, const uint4* d_w2, const LocatePlan& plan,
                                 uint64_t* out_xyzz, size_t n_proofs = 0);
// the one-sum form (the header batch): per non-empty group the XYZZ wire words (16 u64) of sum [w_i] P_i over plan.count device-format points and
// wire weights in the caller's order; the plan uploaded by locate_upload_plan (synchronised)
int32_t locate_group_sums_g1_device(kzg_ctx* ctx, const uint4* d_points, const uint4* d_w, const LocatePlan& plan, uint64_t* out_xyzz);
// batched pairing checks (pairing.hip).  Called under ctx->mu with the device set and the arguments passed through pairing_batch_check_args (host_pairing_batch.h):
// check i is prod e(g1s[k], g2s[k]) over k in [pair_offsets[i], pair_offsets[i + 1]); out_ok: a verdict byte per check, out_gt: 48 u64 per check (the flat GT value,
// zeros for a degenerate check); either may be null; host arrays, written only with KZG_OK.  A point off its curve: the host entry's errors, *bad_index = the pair.
constexpr size_t PAIRING_RUN_MAX_PAIRS = (size_t)1 << 20;        // the most pairs of one call: kzg_host::PAIRING_BATCH_MAX_PAIRS (pairing.hip asserts the two agree)
int32_t pairing_batch_run(kzg_ctx* ctx, const uint64_t* g1s_xy, const uint64_t* g2s, const uint64_t* pair_offsets, size_t n_checks, size_t total, uint8_t* out_ok,
                          uint64_t* out_gt, uint64_t* bad_index);
// hashing on the device (fsdevice.hip).  Called under ctx->mu with the device set.
// count messages of row_len bytes each (host, stride row_len) -> count SHA-256 digests (host); synchronised on return
int32_t sha256_rows_run(kzg_ctx* ctx, const uint8_t* msgs, size_t row_len, size_t count, uint8_t* out_digests);
// The weights r^0 .. r^(count-1) of the coset transcript (host_fiat_shamir.h multiproof_r_powers_host) from values and coset indices ALREADY on the
// device (wire form): commitment rows and proofs go up, the item digests are hashed one lane per item and come back, the one batch hash runs on the
// host, the powers are one product per lane into d_weights (count wire scalars) and are copied to out_r_powers (host).  *fell_back = an input was
// not canonical (a value >= r, a coordinate >= p): nothing is written, the caller derives the weights on the host.  Synchronised on return
int32_t coset_r_powers_device(kzg_ctx* ctx, const uint64_t* commitments, size_t n_commitments, const uint64_t* commitment_indices, const uint4* d_ys,
                              const uint64_t* d_ks, const uint64_t* proofs, size_t count, size_t n, size_t l, uint4* d_weights, uint64_t* out_r_powers,
                              bool* fell_back);
// the same weights from items that are on the device in their SERIALIZED form (d_ys_be: count x l x 32 value bytes, d_proofs_be: count x 32 bytes of
// gnark-compressed proofs; commitments_be and commitment_indices: host): nothing to convert, nothing to fall back from.  Synchronised on return
int32_t coset_r_powers_device_bytes(kzg_ctx* ctx, const uint8_t* commitments_be, size_t n_commitments, const uint64_t* commitment_indices, const uint4* d_ys_be,
                                    const uint64_t* d_ks, const uint4* d_proofs_be, size_t count, size_t n, size_t l, uint4* d_weights, uint64_t* out_r_powers);
// Serialized coset items decoded on the device (cosetbytes.hip, g1_decode.h).  Called under ctx->mu with the device set and slot 0 idle.  Up to two
// arrays of gnark-compressed G1 points (32 B each; [0] commitments, [1] proofs) and one of big-endian scalars (32 B each); an absent array has n = 0.
// The host bytes go up through a ByteStager (byte_stager.h) into ctx->cb (values: cb[0]; points: cb[1]) and stay there (d_*_be).  Points
// leave in the device format of curve.h (d_points, and a second copy at d_points_copy when that is not null) or, with wire_points, as wire points
// with one identity byte each (d_inf); values leave as wire scalars.  bad[a] = index << 2 | kind (G1_BAD_* of g1_decode.h; 0 for a value >= r) of
// the SMALLEST refused index of array a (0 commitments, 1 proofs, 2 values), or 0xFFFFFFFF.
// item_status (the tolerant retriever): refused proofs ([1]) and values do NOT reach bad[1] / bad[2]; every item gets a word of COSET_ITEM_* bits
// instead (d_status, behind the bad words in cb[1]; `status` on the host after the collect), values_per_item values to an item.
constexpr uint32_t COSET_ITEM_PROOF_BYTES = 1, COSET_ITEM_PROOF_OFF_CURVE = 2, COSET_ITEM_VALUE = 4;
struct CosetBytesDecode {
    bool item_status = false;
    size_t values_per_item = 1;                         // a power of two
    uint32_t* d_status = nullptr;                       // (set by the enqueue)
    std::vector<uint32_t> status;                       // (set by the collect)
    const uint8_t* points_be[2] = {nullptr, nullptr};
    size_t n_points[2] = {0, 0};
    uint4* d_points[2] = {nullptr, nullptr};
    uint4* d_points_copy[2] = {nullptr, nullptr};
    uint8_t* d_inf[2] = {nullptr, nullptr};
    bool wire_points = false;
    const uint8_t* ys_be = nullptr;
    size_t n_values = 0;
    uint4* d_ys = nullptr;
    const uint4* d_points_be[2] = {nullptr, nullptr};   // (set by the enqueue)
    const uint4* d_ys_be = nullptr;
    uint32_t bad[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};   // (set by the collect)
};
// uploads and kernels on ctx->stream; the host bytes are consumed on return.  in_use: the stager of a caller that has staged bytes in this call already
struct ByteStager;
int32_t coset_bytes_enqueue(kzg_ctx* ctx, CosetBytesDecode* job, ByteStager* in_use = nullptr);
int32_t coset_bytes_collect(kzg_ctx* ctx, CosetBytesDecode* job);    // drains the stream, reads the three bad words
// the status of a bad word (KZG_OK for 0xFFFFFFFF): KZG_ERR_DESERIALIZE / KZG_ERR_NOT_ON_CURVE, the element's index / per_item to *bad_index (may be
// null), a line with the array's name for kzg_ctx_last_error
int32_t coset_bytes_status(kzg_ctx* ctx, const char* who, const char* array, uint32_t bad_word, size_t per_item, uint64_t* bad_index);
// d_weights[i] = 0 for every item whose status word is not zero (enqueued on ctx->stream)
int32_t coset_mask_refused_weights(kzg_ctx* ctx, uint4* d_weights, const uint32_t* d_status, size_t count);
// Serialized blob headers decoded on the device (headerbytes.hip).  Called under ctx->mu with the device set and slot 0 idle; count <= 2^20.  Per
// header 32 B of gnark-compressed commitment and 64 B each of length commitment and length proof (g2_decode.h's format and the identity 0x40 || 63
// zeros), staged through ONE ByteStager (byte_stager.h) into ws.bases_wire (G2) and ctx->cb[1] (G1), where they stay.  The G2 elements
// leave subgroup-checked at d_g2: the device format of curve_g2.h in the order C2_0, pi2_0, C2_1, .. or, with `wire`, wire points, the count C2 in
// front of the count pi2 (the identity as zeros either way).  The commitments leave at d_commitments in the device format of curve.h or, with `wire`,
// as wire points with one identity byte each at d_commitments_inf.  bad_g1 = index << 2 | kind (G1_BAD_* of g1_decode.h) of the smallest refused
// commitment, bad_g2 = (2 header + (0 C2, 1 pi2)) << 2 | kind (G2_BAD_* of g2_decode.h) of the smallest refused element, or 0xFFFFFFFF.
struct HeaderBytesDecode {
    const uint8_t *commitments_be = nullptr, *length_commitments_be = nullptr, *length_proofs_be = nullptr;
    size_t count = 0;
    bool wire = false;
    uint4* d_commitments = nullptr;
    uint8_t* d_commitments_inf = nullptr;
    uint4* d_g2 = nullptr;
    const uint4* d_commitments_be = nullptr;       // (set by the decode)
    uint32_t bad_g1 = 0xFFFFFFFFu, bad_g2 = 0xFFFFFFFFu;
};
int32_t header_bytes_decode(kzg_ctx* ctx, HeaderBytesDecode* job);   // synchronised on return
// the status of its two bad words (KZG_OK when both are 0xFFFFFFFF), a bad commitment first: KZG_ERR_DESERIALIZE / KZG_ERR_NOT_ON_CURVE, the header to
// *bad_index and 0 / 1 / 2 (commitment, length commitment, length proof) to *bad_array (both may be null), a line for kzg_ctx_last_error
int32_t header_bytes_status(kzg_ctx* ctx, const char* who, const HeaderBytesDecode& job, uint64_t* bad_index, int32_t* bad_array);
// the item digests of the header transcript (host_fiat_shamir.h header_item_message), one lane per header, from the commitments' bytes and the decoded
// G2 points where header_bytes_decode left them (device format); claimed_lens and out_digests (32 B per header): host.  Uses ctx->fs.  Synchronised on return
int32_t header_item_digests_run(kzg_ctx* ctx, const uint4* d_commitments_be, const uint4* d_g2, const uint64_t* claimed_lens, size_t count, uint8_t* out_digests);
// selected cosets (provecosets.hip): per item (poly_indices[i] or 0, coset_indices[i]) the quotient row (out_q: d wire words), the l values (out_ys) and the
// proof (out_xy, out_inf; needs srs), each optional; rows bit-identical to multiproof_encode's.  Called under ctx->mu with the device set, the arguments checked,
// plan.n_items > 0 and slot 0 idle; synchronised on return
int32_t prove_cosets_run(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* polys_mont, size_t count, bool eval_form, const ProveCosetsPlan& plan,
                         const uint64_t* poly_indices, const uint64_t* coset_indices, uint64_t* out_q, uint64_t* out_ys, uint64_t* out_xy, uint8_t* out_inf);
// erasure decoding (recover.hip): the polynomial of degree < count l through the values of the plan's cosets (ys: host, count x l wire values), as n
// coefficients or evaluations on the host; *consistent = its coefficients from plan.degree_bound on are zero.  Called under ctx->mu, synchronised on return
int32_t recover_run(kzg_ctx* ctx, const RecoverPlan& plan, const uint64_t* ys, bool eval_form, uint64_t* out_poly, int32_t* consistent);
// Where a batch takes its values (blobs x count x l, 32 B each) and how its rows (blobs x plan.out_len, 32 B each) leave
struct RecoverIo {
    const void* ys = nullptr;          // host values, staged group by group; ignored when d_ys is set
    const uint4* d_ys = nullptr;       // or: the values where they lie on the device (valid on ctx->stream), no upload
    bool ys_be = false;                // the values are 32-byte big-endian integers (decoded on load), not wire words
    void* out = nullptr;               // host rows
    bool out_be = false;               // ... as 32-byte big-endian integers, not wire words
    int32_t* consistent = nullptr;     // blobs flags or null
    uint32_t* bad_word = nullptr;      // ys_be, KZG_ERR_DESERIALIZE: (the smallest index of a value >= r) << 2, for coset_bytes_status; may be null
};
// the same for the plan's blobs, group by group, every stage one launch per group; recover_run is the batch of one on host words.  With ys_be a value
// >= r ends the call at its group with KZG_ERR_DESERIALIZE (rows up to that group may have been written; needs blobs x count x l <= 2^28)
int32_t recover_run_batch(kzg_ctx* ctx, const RecoverBatchPlan& plan, const RecoverIo& io);

// polynomial pipeline (poly.hip)
int32_t proof_run(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* evals, size_t n, const uint64_t z[4],
                  uint64_t out_xy[8], uint8_t* out_inf, uint64_t* out_y, bool want_proof, size_t coeff_lo, uint64_t* out_xyzz);
int32_t proof_begin(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* evals, size_t n, const uint64_t z[4], int slot, const void* d_resident = nullptr);
int32_t proof_end(kzg_ctx* ctx, int slot, uint64_t out_xy[8], uint8_t* out_inf, uint64_t* out_y);
int32_t roots_run(kzg_ctx* ctx, uint64_t* out, size_t n);
int32_t blob_to_fr_run(kzg_ctx* ctx, const uint8_t* bytes, size_t len, size_t n_padded, void** d_out,
                       hipStream_t st = nullptr, DeviceBuffer* d_bytes = nullptr, DeviceBuffer* d_elems = nullptr);
// the batched evaluations of batch verification (vbeval.hip k_vb_prep / k_vb_eval), one workgroup per blob of up to 2^VB_MAX_LOG elements;
// larger blobs take the single-polynomial path.  VbBlob describes a blob to the host driver and to the kernels alike.
constexpr int VB_MAX_LOG = 12;
struct VbBlob { uint64_t off; uint32_t len; uint32_t log_n; };          // byte offset (32-byte aligned, zero-filled to the next chunk), byte length, log2(padded elements)
static_assert(sizeof(VbBlob) == 16, "descriptors are uploaded as they are");
int32_t vb_evaluate_setup(kzg_ctx* ctx, size_t packed_len, size_t nb);
int32_t vb_evaluate_enqueue(kzg_ctx* ctx, const uint8_t* packed, const VbBlob* meta, size_t nb, size_t b0, size_t b1, const uint64_t* zs,
                            uint8_t* small_pinned);
int32_t vb_evaluate_finish(kzg_ctx* ctx, size_t nb, uint64_t* ys_out, uint8_t* fallback_out);
// the batched prover (provebatch.hip), one launch sequence per group of rows of one length class n = 2^log_n <= 2^PROVE_BATCH_MAX_LOG; the caller holds
// ctx->mu, has set the device and found every slot idle.  prove_batch_rows_from_bytes: `rows` blobs packed in host memory (blob r at meta[r].off, 32-byte
// aligned, zero-filled to its last whole element) -> rows x n wire elements in ctx->pb[1] (helpers::to_fr_array, zero padding to n), enqueued on ctx->stream.
// prove_batch_rows_run: rows x n wire evaluations on the device (written on ctx->stream or complete) and `rows` points (host, wire) -> y_b = f_b(z_b) and the
// proof of every row, its quotient's commitment over `basis`, the cached Lagrange basis of n points; out_inf / out_ys may be null.
int32_t prove_batch_rows_from_bytes(kzg_ctx* ctx, const uint8_t* packed, size_t packed_bytes, const VbBlob* meta, size_t rows, int log_n, const void** d_rows);
int32_t prove_batch_rows_run(kzg_ctx* ctx, kzg_srs* basis, const void* d_rows, int log_n, size_t rows, const uint64_t* zs, uint64_t* out_xy, uint8_t* out_inf,
                             uint64_t* out_ys);
// Lagrange-sharded proofs (lagrange.hip; the host folds lag_fold_y / lag_fold_proof: host_lagrange.h)
int32_t lag_begin(kzg_ctx* ctx, const kzg_srs* shard, size_t base, const void* evals, bool on_device, size_t len, size_t n, const uint64_t z[4], int slot, int commit_slot);
int32_t lag_partial_y(kzg_ctx* ctx, int slot, uint64_t out[8]);
int32_t lag_continue(kzg_ctx* ctx, int slot, const uint64_t y[4]);
int32_t lag_end(kzg_ctx* ctx, int slot, uint64_t out_part[32], uint64_t* out_commit);
void lag_abort(kzg_ctx* ctx, int slot);
int32_t lag_quotient_eval_on_domain(kzg_ctx* ctx, const uint64_t z[4], const uint64_t* evals, size_t n, const uint64_t value[4], uint64_t out[4]);

// MSM front ends shared by the units of the C-ABI (capi.hip).  _locked: the caller holds ctx->mu (msm_g1_batch_locked: and has set the device).
// off_curve != nullptr: the uploaded points are validated on the device, *off_curve = 1 if one fails (then no MSM runs over them)
int32_t msm_srs_locked(kzg_ctx* ctx, const kzg_srs* srs, size_t offset, const void* scalars, bool on_device, size_t n,
                       uint64_t out_xy[8], uint8_t* out_inf, uint64_t* out_xyzz);
int32_t msm_g1_batch_locked(kzg_ctx* ctx, const uint64_t* bases_xy_mont, const uint64_t* scalars_mont, size_t n, size_t batch,
                            uint64_t* out_xy_mont, uint8_t* out_is_infinity, uint32_t* off_curve);
int32_t msm_g1_batch_impl(kzg_ctx* ctx, const uint64_t* bases_xy_mont, const uint64_t* scalars_mont, size_t n, size_t batch,
                          uint64_t* out_xy_mont, uint8_t* out_is_infinity, uint32_t* off_curve);
// `count` polynomials of n coefficients each (device, wire form, one after the other) committed over the first n points of one SRS as ONE
// MSM problem (capi.hip: the body of kzg_commit_coeff_form_batch_device; builds the SRS's per-bit tables on first use).  The caller holds
// ctx->mu, has set the device, and the scalars are complete (the launches run on the slots' streams)
int32_t commit_batch_device(kzg_ctx* ctx, kzg_srs* basis, const void* d_scalars, size_t n, size_t count, uint64_t* out_xy, uint8_t* out_inf);
// wire points of the host -> device format at d_out through `staging`, synchronised on return (capi_srs.hip)
int32_t upload_points(kzg_ctx* ctx, const uint64_t* xy, size_t n, uint4* d_out, DeviceBuffer& staging, uint32_t* off_curve = nullptr);

int32_t set_error(kzg_ctx* ctx, hipError_t e, const char* where);
// true (and the line for kzg_ctx_last_error) while a kzg_*_begin holds slot 0's buffers, which the synchronous entries work in; names_msm_end: the text of msm.hip
inline bool slot0_refused(kzg_ctx* ctx, bool names_msm_end = false) {
    if (ctx->slot_pending[0]) ctx->last_error = std::string("a kzg_*_begin on slot 0 is still in flight: call ") + (names_msm_end ? "kzg_msm_g1_srs_end(ctx, 0, ..)" : "its end") + " first";
    return ctx->slot_pending[0] != nullptr;
}
// shared by the verifier units (defined in capi_verify.hip, used there and in capi_coset.hip): the G2 point of a pairing check (nullptr: consts::G2_TAU;
// false = not on the twist), helpers::pairings_verify with the two Miller loops on the host pool, the clock of the KZG_VB_TRACE lines
using Clock = std::chrono::steady_clock;
inline double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
bool load_g2_tau(const uint64_t* g2_tau_mont, kzg_host::G2* out);
bool pairings_verify_pooled(const kzg_host::G1& a1, const kzg_host::G2& a2, const kzg_host::G1& b1, const kzg_host::G2& b2);
// the context's high-priority auxiliary stream (lagrange.hip)
int32_t ctx_aux_stream(kzg_ctx* ctx, hipStream_t fallback, hipStream_t* out);
// the points only, no window / per-bit tables (set-up paths that need the points once: kzg_multi_cache_lagrange)
int32_t srs_upload_plain(kzg_ctx* ctx, const uint64_t* g1_xy_mont, size_t n_points, kzg_srs** out);

// job(i) for i < n on the library's persistent host pool (host_pool.h HostPool, sized in runtime.hip; the calling thread takes part)
void host_parallel_for(size_t n, const std::function<void(size_t)>& job);
unsigned host_pool_threads(size_t jobs);   // threads such a call of `jobs` jobs runs on (traces)
// joins the transcript threads and frees the buffers of the blob stream (kzg_ctx_destroy)
void blob_stream_release(kzg_ctx* ctx);

// Every environment variable the library reads (runtime.hip opts(); header: "ENVIRONMENT").  Read once per process, except the two SRS switches,
// which are read at every upload so that a host can load one SRS with and one without tables (bench.py does).
struct Opts {
    int host_threads_max = 0;        // KZG_HOST_THREADS_MAX: cap of the host pool (transcripts of batch verification); 0 = min(48, the cgroup's CPU quota)
    int host_threads = 0;            // KZG_HOST_THREADS: exactly that many pool threads (measurements)
    int vb_trace = 0;                // KZG_VB_TRACE: 1 = phase times of batch verification on stderr, 2 = per upload chunk
    size_t vb_group_bytes = 0;       // KZG_VB_GROUP_BYTES: packed blob bytes per GPU round of batch verification (default 256 MiB)
    size_t vb_chunk_bytes = 0;       // KZG_VB_CHUNK_BYTES: bytes per upload chunk inside a round (default 16 MiB)
    bool roctx = false;              // KZG_ROCTX: roctx ranges around the host phases (rocprofv3 --marker-trace)
    double exchange_timeout_s = 60;  // KZG_EXCHANGE_TIMEOUT_S: bound of the wait for a collective of the _rccl entries
    const char* rccl_lib = nullptr;  // KZG_RCCL_LIB: the RCCL to dlopen instead of the one already in the process
    int ntt_tile_log = 0;            // KZG_NTT_TILE_LOG: 10 / 11 = one NTT tile size at every transform size (0: by size)
};
const Opts& opts();
bool opt_no_precompute();            // KZG_NO_PRECOMPUTE=1: SRS uploads build no window tables (and no per-bit tables): 64 B per point
bool opt_no_naf();                   // KZG_NO_NAF=1: SRS uploads build no per-bit tables (16 KiB per point saved; fixed-window MSMs)

// process-wide caches keyed by device (NTT twiddles, g1_ifft scalar sets): released when the LAST context of a device is destroyed
void ntt_release_device_caches(int dev);
void g1fft_release_device_caches(int dev);

}  // namespace kzg

// ---- roctx phase ranges (tracing) ------------------------------------------------------------------------
// KZG_ROCTX=1 makes the library mark its host-side phases (enqueue of the sort / accumulate / reduction kernels of an MSM, the host
// epilogue, NTT, proof pipeline, the stages of batch verification) with roctx ranges, visible in `rocprofv3 --marker-trace`.  The
// marker library (librocprofiler-sdk-roctx.so, else libroctx64.so) is loaded with dlopen on first use: no link-time dependency,
// no cost when the variable is unset.
namespace kzg {
void roctx_push(const char* name);
void roctx_pop();
struct RoctxRange {
    explicit RoctxRange(const char* name) { roctx_push(name); }
    ~RoctxRange() { roctx_pop(); }
    RoctxRange(const RoctxRange&) = delete;
    RoctxRange& operator=(const RoctxRange&) = delete;
};
struct RoctxPhases {             // consecutive phases of one function; whatever is open closes on every return path
    bool open = false;
    void begin(const char* name) { end(); roctx_push(name); open = true; }
    void end() { if (open) { roctx_pop(); open = false; } }
    ~RoctxPhases() { end(); }
};
}  // namespace kzg

#define KZG_HIP_TRY(ctx, expr)                                                     \
    do {                                                                           \
        hipError_t _e = (expr);                                                    \
        if (_e != hipSuccess) return kzg::set_error((ctx), _e, #expr);             \
    } while (0)
