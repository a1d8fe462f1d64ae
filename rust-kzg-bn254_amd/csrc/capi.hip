// capi.hip — the C-ABI of include/kzg_bn254_mi355x.h: contexts, MSM, NTT, commitments, proofs, challenges.  Plain pointers and sizes only.
// (The SRS surface: capi_srs.hip; the verifiers: capi_verify.hip, capi_coset.hip; environment, host pool, error text: runtime.hip.)
#include "engine.h"
#include "host_curve.h"
#include "host_pairing.h"
#include "host_sha256.h"
#include "host_fiat_shamir.h"
#include "host_lagrange.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <thread>

using namespace kzg;
using kzg_host::blob_padded_len;
using kzg_host::next_pow2;

namespace {
// live contexts per device: the caches of ntt.hip / g1fft.hip outlive a context (they are shared by the contexts of a device) and are
// freed with the last one (they were never freed)
std::mutex g_ctx_count_mu;
std::map<int, int> g_ctx_count;

// ---- MSM ------------------------------------------------------------------------------------------
int32_t stage_scalars(kzg_ctx* ctx, const uint64_t* scalars, size_t n, const void** d_out) {
    KZG_HIP_TRY(ctx, ctx->msm.scalars.reserve(n * 32 + 32));
    if (n) KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->msm.scalars.p, scalars, n * 32, hipMemcpyHostToDevice, ctx->stream));
    *d_out = ctx->msm.scalars.p;
    return KZG_OK;
}
void write_identity(uint64_t out_xy[8], uint8_t* out_inf, uint64_t* out_xyzz) {
    if (out_xy) memset(out_xy, 0, 64);
    if (out_inf) *out_inf = 1;
    if (out_xyzz) memset(out_xyzz, 0, 128);
}

constexpr size_t MSM_SPLIT_MAX = (size_t)1 << 21;     // halves of up to 2^20 pairs: one launch each
}  // namespace

namespace kzg {
// (the caller holds ctx->mu and has set the device)
int32_t msm_g1_batch_locked(kzg_ctx* ctx, const uint64_t* bases_xy_mont, const uint64_t* scalars_mont, size_t n, size_t batch,
                                   uint64_t* out_xy_mont, uint8_t* out_is_infinity, uint32_t* off_curve) {
    if (off_curve) *off_curve = 0;
    if (n == 0) {
        for (size_t i = 0; i < batch; ++i) write_identity(out_xy_mont + 8 * i, out_is_infinity ? out_is_infinity + i : nullptr, nullptr);
        return KZG_OK;
    }
    const size_t total = n * batch;
    KZG_HIP_TRY(ctx, ctx->msm.bases.reserve(total * 64));
    int32_t rc = upload_points(ctx, bases_xy_mont, total, ctx->msm.bases.as<uint4>(), ctx->msm.bases_wire, off_curve);
    if (rc != KZG_OK) return rc;
    if (off_curve && *off_curve) return KZG_OK;              // the caller reports the invalid point; no MSM over it
    const void* d_scalars;
    rc = stage_scalars(ctx, scalars_mont, total, &d_scalars);
    if (rc != KZG_OK) return rc;
    return msm_run_batch(ctx, ctx->msm.bases.as<uint4>(), d_scalars, n, (uint32_t)batch, out_xy_mont, out_is_infinity);
}
int32_t msm_g1_batch_impl(kzg_ctx* ctx, const uint64_t* bases_xy_mont, const uint64_t* scalars_mont, size_t n, size_t batch,
                                 uint64_t* out_xy_mont, uint8_t* out_is_infinity, uint32_t* off_curve) {
    if (!ctx || !out_xy_mont || batch == 0 || batch > 64) return KZG_ERR_INVALID_ARG;
    if (n && (!bases_xy_mont || !scalars_mont)) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return msm_g1_batch_locked(ctx, bases_xy_mont, scalars_mont, n, batch, out_xy_mont, out_is_infinity, off_curve);
}

// (the caller holds ctx->mu)
int32_t msm_srs_locked(kzg_ctx* ctx, const kzg_srs* srs, size_t offset, const void* scalars, bool on_device, size_t n,
                              uint64_t out_xy[8], uint8_t* out_inf, uint64_t* out_xyzz) {
    if (!ctx || !srs || srs->ctx->device != ctx->device || (!out_xy && !out_xyzz)) return KZG_ERR_INVALID_ARG;   // an SRS may be shared by the contexts of its GPU
    if (n && !scalars) return KZG_ERR_INVALID_ARG;
    if (offset > srs->n || n > srs->n - offset) return KZG_ERR_MSM_LENGTH_MISMATCH;
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n == 0) { write_identity(out_xy, out_inf, out_xyzz); return KZG_OK; }
    const void* d_scalars = scalars;
    if (!on_device) {
        // A large MSM from a HOST buffer, one call at a time: as TWO halves on two slots.  The upload of the second half (a pageable copy: this
        // thread sits in it) runs beside the kernels of the first half, and the first half's accumulate beside the second half's sort; the two
        // partial sums are added on the host.  Resident, two halves cost what the whole costs (tools/probe_split_lone.py: 2^19 0.872 against
        // 0.887 ms, 2^20 1.444 against 1.445) -- so the hidden part of the upload is the gain: 2^19 1.15 -> 1.07 ms, 2^20 2.00 -> 1.76.
        // Below 2^19 pairs the second bucket set costs more than the hidden copy (2^18: 0.601 against 0.553 resident).
        // share of the FIRST half (the smaller it is, the sooner the GPU starts and the more of the upload is hidden; too small and the second MSM runs alone):
        // measured from host buffers, 0.375 / 0.44 / 0.5 / 0.56: 2^19 1.116 / 1.070 / 1.084 / 1.111 ms (unsplit 1.148), 2^20 1.756 / 1.786 / 1.901 / 1.863 (unsplit 2.000)
        const double split_frac = n >= ((size_t)1 << 20) ? 0.375 : 0.44;
        const bool idle = !ctx->slot_pending[0] && !ctx->slot_pending[1] && ctx->lag[0].phase == 0 && ctx->lag[1].phase == 0;
        if (idle && n >= ((size_t)1 << 19) && n <= MSM_SPLIT_MAX && ctx->msm_c_override == 0 && srs_bits(srs)) {
            const size_t half = ((size_t)((double)n * split_frac) + 255) / 256 * 256;
            const uint64_t* sc = static_cast<const uint64_t*>(scalars);
            const size_t lo[2] = {0, half}, len[2] = {half, n - half};
            int32_t rc = KZG_OK;
            int begun = 0;
            for (int h = 0; h < 2 && rc == KZG_OK; ++h) {
                hipStream_t st = nullptr;
                rc = msm_slot_stream(ctx, h, &st);
                if (rc != KZG_OK) break;
                MsmWorkspace& ws = ctx->slot_msm(h);
                hipError_t e = ws.scalars.reserve(len[h] * 32 + 32);
                if (e == hipSuccess) e = hipMemcpyAsync(ws.scalars.p, sc + 4 * lo[h], len[h] * 32, hipMemcpyHostToDevice, st);
                if (e != hipSuccess) { rc = set_error(ctx, e, "split upload"); break; }
                rc = msm_begin(ctx, h, srs_bases(srs, offset + lo[h], len[h], true), ws.scalars.p, len[h]);
                if (rc == KZG_OK) ++begun;
            }
            kzg_host::Xyzz parts[2] = {kzg_host::xyzz_inf(), kzg_host::xyzz_inf()};
            for (int h = 0; h < begun; ++h) {                          // (also after a failure of the second half: nothing may stay in flight)
                uint64_t w[16];
                const int32_t r2 = msm_end(ctx, h, nullptr, nullptr, w);
                if (r2 == KZG_OK) memcpy(&parts[h], w, 128); else if (rc == KZG_OK) rc = r2;
            }
            if (rc != KZG_OK) return rc;
            const kzg_host::Xyzz total = kzg_host::xyzz_add(parts[0], parts[1]);
            if (out_xyzz) memcpy(out_xyzz, &total, 128);
            if (out_xy) kzg_host::xyzz_to_affine(total, out_xy, out_inf);
            return KZG_OK;
        }
        int32_t rc = stage_scalars(ctx, static_cast<const uint64_t*>(scalars), n, &d_scalars);
        if (rc != KZG_OK) return rc;
    }
    return msm_run(ctx, srs_bases(srs, offset, n, ctx->msm_c_override == 0), d_scalars, n, out_xy, out_inf, out_xyzz);
}
}  // namespace kzg

namespace {
int32_t msm_srs_common(kzg_ctx* ctx, const kzg_srs* srs, size_t offset, const void* scalars, bool on_device, size_t n,
                              uint64_t out_xy[8], uint8_t* out_inf, uint64_t* out_xyzz) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return msm_srs_locked(ctx, srs, offset, scalars, on_device, n, out_xy, out_inf, out_xyzz);
}

// ---- batched commitments: `count` polynomials of n coefficients / evaluations over one SRS in ONE kernel sequence -------------------
// The reference commits one blob per call (kzg.rs:84-125); a service that commits many small blobs pays the fixed depth of an MSM
// (~0.14-0.2 ms at 512..2048 coefficients: sort, ~13 dependent point additions, host epilogue) per blob.  Here the polynomials share the
// bases, so they are one MSM problem: width-8 NAF digits over the SRS's per-bit tables, 64 buckets per polynomial in one bucket
// array (msm.hip msm_run_batch_tables).  An SRS without per-bit tables (fewer than 2^15 points) gets them on the first batched call.
}  // namespace
namespace kzg {
int32_t commit_batch_device(kzg_ctx* ctx, kzg_srs* basis, const void* d_scalars, size_t n, size_t count, uint64_t* out_xy, uint8_t* out_inf) {
    uint4* bits = srs_bits(basis);
    if (!bits) {
        int32_t rc = srs_build_bit_tables(ctx, basis, true);
        if (rc != KZG_OK) return rc;
        bits = srs_bits(basis);
    }
    if (!bits) {                                  // no room for tables (or KZG_NO_NAF): one commitment after the other
        for (size_t k = 0; k < count; ++k) {
            int32_t rc = msm_run(ctx, srs_bases(basis, 0, n, ctx->msm_c_override == 0), static_cast<const char*>(d_scalars) + k * n * 32, n,
                                 out_xy + 8 * k, out_inf ? out_inf + k : nullptr, nullptr);
            if (rc != KZG_OK) return rc;
        }
        return KZG_OK;
    }
    MsmBases b;
    b.points = bits; b.table_stride = (uint32_t)basis->n; b.c = 7; b.W = 255; b.naf = true;
    return msm_run_batch_tables(ctx, b, d_scalars, n, count, out_xy, out_inf);
}
}  // namespace kzg
namespace {
int32_t commit_batch_common(kzg_ctx* ctx, kzg_srs* srs, const void* scalars, bool on_device, bool eval_form, size_t n, size_t count,
                                   uint64_t* out_xy, uint8_t* out_inf) {
    if (!ctx || !srs || srs->ctx != ctx || !out_xy || (n && count && !scalars)) return KZG_ERR_INVALID_ARG;
    if (n > srs->n) return eval_form ? KZG_ERR_SRS_CAPACITY_EXCEEDED : KZG_ERR_POLY_LENGTH;          // kzg.rs:89-94, :112-116
    if (eval_form && (n == 0 || (n & (n - 1)) != 0)) return KZG_ERR_NOT_POWER_OF_TWO;                // kzg.rs:265-269
    if (count == 0) return KZG_OK;
    if (n == 0) { memset(out_xy, 0, count * 64); if (out_inf) memset(out_inf, 1, count); return KZG_OK; }
    if (count > ((size_t)1 << 40) / n) return KZG_ERR_TOO_LARGE;
    kzg_srs* basis = srs;
    if (eval_form) {                                       // the reference's literal form: MSM over the Lagrange basis of n points, kept with the SRS
        int32_t rc = kzg_srs_cache_lagrange(ctx, srs, n);
        if (rc != KZG_OK) return rc;
        basis = srs_cached_lagrange(srs, n);
        if (!basis) return KZG_ERR_INVALID_ARG;             // dropped by another thread between the two calls
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const void* d = scalars;
    if (!on_device) {
        KZG_HIP_TRY(ctx, ctx->msm.scalars.reserve(count * n * 32 + 32));
        KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->msm.scalars.p, scalars, count * n * 32, hipMemcpyHostToDevice, ctx->stream));
        KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // the launches run on the slots' streams
        d = ctx->msm.scalars.p;
    }
    return commit_batch_device(ctx, basis, d, n, count, out_xy, out_inf);
}

int32_t lagrange_begin_common(kzg_ctx* ctx, const kzg_srs* shard, size_t lo, const void* evals, bool on_device, size_t len, size_t n,
                                     const uint64_t z[4], int32_t slot, int32_t commit_slot = -1) {
    if (!ctx || !shard || shard->ctx->device != ctx->device || !z || (len && !evals)) return KZG_ERR_INVALID_ARG;
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_INVALID_INPUT_LENGTH;           // helpers.rs:485-487
    if (n > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    if (lo > n || len > n - lo) return KZG_ERR_INVALID_ARG;
    if (len > shard->n) return KZG_ERR_SRS_CAPACITY_EXCEEDED;                        // kzg.rs:89-94 (commit_eval_form of the quotient)
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return lag_begin(ctx, shard, lo, evals, on_device, len, n, z, slot, commit_slot);
}

// asynchronous forms of commit_eval_form / commit_blob: the whole chain (H2D, bytes -> Fr, IFFT, MSM) goes onto the slot's stream
int32_t commit_begin_common(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* evals_mont, const uint8_t* blob_bytes, size_t len,
                                   size_t n, int32_t slot) {
    if (slot < 0 || slot >= KZG_NUM_SLOTS) return KZG_ERR_INVALID_ARG;
    if (n > srs->n) return KZG_ERR_SRS_CAPACITY_EXCEEDED;                            // kzg.rs:89-94
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_NOT_POWER_OF_TWO;
    if (n > ((size_t)1 << 24)) return KZG_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->slot_pending[slot]) return KZG_ERR_INVALID_ARG;
    hipStream_t st = nullptr;
    int32_t rc = msm_slot_stream(ctx, slot, &st);
    if (rc != KZG_OK) return rc;
    MsmWorkspace& ws = ctx->slot_msm(slot);
    void* d = nullptr;
    if (blob_bytes || !evals_mont) {
        rc = blob_to_fr_run(ctx, blob_bytes, len, n, &d, st, &ws.blob, &ws.scalars);
        if (rc != KZG_OK) return rc;
    } else {
        KZG_HIP_TRY(ctx, ws.scalars.reserve(n * 32 + 32));
        KZG_HIP_TRY(ctx, hipMemcpyAsync(ws.scalars.p, evals_mont, n * 32, hipMemcpyHostToDevice, st));
        d = ws.scalars.p;
    }
    if (const kzg_srs* cached = srs_cached_lagrange(srs, n))                         // no IFFT: MSM over the cached Lagrange basis
        return msm_begin(ctx, slot, srs_bases(cached, 0, n, ctx->msm_c_override == 0), d, n);
    NttTables tb;                                                                    // make sure the tables exist before the slot stream reads them
    const int log_n = ilog2_ceil(n);
    if (n > 1) { rc = ntt_get_tables(ctx, log_n, true, &tb); if (rc != KZG_OK) return rc; }
    rc = ntt_run(ctx, d, n, true, st, &ctx->slot_ntt(slot));
    if (rc != KZG_OK) return rc;
    return msm_begin(ctx, slot, srs_bases(srs, 0, n, ctx->msm_c_override == 0), d, n);
}

// shared body: `commitment_in` given (compute_blob_proof) or computed here beside the transcript hash (commit + proof)
int32_t blob_proof_common(kzg_ctx* ctx, const kzg_srs* srs, const uint8_t* blob_bytes, size_t len, size_t n_roots,
                                 const uint64_t* commitment_in, uint64_t* out_commitment_xy, uint8_t* out_commitment_inf,
                                 uint64_t out_proof_xy[8], uint8_t* out_proof_inf, uint64_t* out_z_mont, uint64_t* out_y_mont) {
    if (!ctx || !srs || srs->ctx != ctx || !out_proof_xy || (len && !blob_bytes)) return KZG_ERR_INVALID_ARG;
    const size_t n_elems = (len + 31) / 32;
    if (n_elems > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;                       // polynomial.rs:42-46
    const size_t n = blob_padded_len(len);
    kzg_host::G1 commitment;
    if (commitment_in) {
        commitment = kzg_host::g1_from_wire(commitment_in);
        if (!kzg_host::g1_on_curve(commitment)) return KZG_ERR_G1_NOT_ON_CURVE;      // kzg.rs:295
    }
    if (n != n_roots) return KZG_ERR_ROOTS_LENGTH;                                   // kzg.rs:135-139 (compute_proof_impl)
    if (n > srs->n) return KZG_ERR_SRS_CAPACITY_EXCEEDED;                            // kzg.rs:89-94 (commit_eval_form of the quotient)
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_refused(ctx)) return KZG_ERR_INVALID_ARG;
    // the transcript prefix does not depend on the commitment: hash it on a host thread while the GPU works
    kzg_host::Sha256 sh;
    kzg_host::sha256_init(sh);
    std::thread hasher([&] { challenge_absorb_prefix(sh, blob_bytes, len, n); });
    struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{hasher};
    PolySet& set = ctx->poly[0];
    void* d_evals = nullptr;
    int32_t rc = blob_to_fr_run(ctx, blob_bytes, len, n, &d_evals, ctx->stream, &set.c, &set.a);    // evaluations (wire) in set.a
    if (rc != KZG_OK) return rc;
    if (!commitment_in) {
        // commit_blob on a copy of the evaluations (the IFFT is in place); runs beside the hash
        uint64_t cxy[8]; uint8_t cinf = 0;
        if (const kzg_srs* cached = srs_cached_lagrange(srs, n)) {                   // the evaluations themselves are the scalars: no copy, no IFFT
            rc = msm_run(ctx, srs_bases(cached, 0, n, ctx->msm_c_override == 0), d_evals, n, cxy, &cinf, nullptr);
        } else {
            KZG_HIP_TRY(ctx, ctx->msm.scalars.reserve(n * 32 + 32));
            KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->msm.scalars.p, d_evals, n * 32, hipMemcpyDeviceToDevice, ctx->stream));
            rc = ntt_run(ctx, ctx->msm.scalars.p, n, true);
            if (rc != KZG_OK) return rc;
            rc = msm_run(ctx, srs_bases(srs, 0, n, ctx->msm_c_override == 0), ctx->msm.scalars.p, n, cxy, &cinf, nullptr);
        }
        if (rc != KZG_OK) return rc;
        commitment = kzg_host::g1_from_wire(cxy);
        if (out_commitment_xy) memcpy(out_commitment_xy, cxy, 64);
        if (out_commitment_inf) *out_commitment_inf = cinf;
    }
    hasher.join();
    uint64_t z[4];
    challenge_finish(sh, commitment, z);
    if (out_z_mont) memcpy(out_z_mont, z, 32);
    return proof_run(ctx, srs, nullptr, n, z, out_proof_xy, out_proof_inf, out_y_mont, true, 0, nullptr);   // evaluations already in set.a
}
}  // namespace

extern "C" {

const char* kzg_status_message(int32_t status) {
    switch (status) {
        case KZG_OK: return "ok";
        case KZG_ERR_INVALID_ARG: return "invalid argument";
        case KZG_ERR_NO_DEVICE: return "no HIP device available (this library has no CPU fallback)";
        case KZG_ERR_DEVICE: return "HIP runtime error";
        case KZG_ERR_MSM_LENGTH_MISMATCH: return "MSM Error: bases and scalars have different lengths";
        case KZG_ERR_SRS_CAPACITY_EXCEEDED: return "SRS capacity exceeded";
        case KZG_ERR_POLY_LENGTH: return "polynomial length is not correct";
        case KZG_ERR_NOT_POWER_OF_TWO: return "length provided is not a power of 2";
        case KZG_ERR_DOMAIN: return "Could not perform IFFT due to domain consturction error";
        case KZG_ERR_ROOTS_LENGTH: return "inconsistent length between blob and root of unities";
        case KZG_ERR_INVALID_INPUT_LENGTH: return "Invalid input length";
        case KZG_ERR_TOO_LARGE: return "Input size exceeds maximum polynomial size";
        case KZG_ERR_ROOT_NOT_FOUND: return "Root of unity not found";
        case KZG_ERR_ZERO_LENGTH: return "Length of data after padding is 0";
        case KZG_ERR_SRS_LENGTH: return "the length of data after padding is not valid with respect to the SRS";
        case KZG_ERR_DESERIALIZE: return "point at infinity not coded properly for g1";
        case KZG_ERR_NOT_ON_CURVE: return "compressed g1 point not on curve";
        case KZG_ERR_G1_NOT_ON_CURVE: return "G1 point not on curve";
        case KZG_ERR_G2_TAU_NOT_ON_CURVE: return "Invalid trusted setup: G2_TAU not on curve";
        case KZG_ERR_TAU_EQUALS_Z: return "Evaluation point equals trusted setup secret";
        case KZG_ERR_PEER: return "another rank of the communicator failed in this collective call";
        case KZG_ERR_EXCHANGE_TIMEOUT: return "the exchange between the ranks timed out";
        case KZG_ERR_IO: return "file could not be read or written";
        default: return "unknown status";
    }
}

int32_t kzg_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int32_t kzg_ctx_create(int32_t device_id, kzg_ctx** out) {
    if (!out) return KZG_ERR_INVALID_ARG;
    *out = nullptr;
    int n = kzg_device_count();
    if (n <= 0 || device_id < 0 || device_id >= n) return KZG_ERR_NO_DEVICE;
    if (hipSetDevice(device_id) != hipSuccess) { (void)hipGetLastError(); return KZG_ERR_NO_DEVICE; }
    kzg_ctx* ctx = new (std::nothrow) kzg_ctx();
    if (!ctx) return KZG_ERR_INVALID_ARG;
    ctx->device = device_id;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0)
            ctx->acc_wave_slots = (uint32_t)cus * 4u * 3u;                // k_msm_accumulate: 3 waves per SIMD (KZG_ACC_WAVES)
        else (void)hipGetLastError();
    }
    {
        std::lock_guard<std::mutex> lk(g_ctx_count_mu);          // (taken before the handle exists: no call on it can reach a cache that kzg_ctx_destroy is freeing)
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); delete ctx; return KZG_ERR_DEVICE; }
        ++g_ctx_count[device_id];
    }
    *out = ctx;
    return KZG_OK;
}

void kzg_ctx_destroy(kzg_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    blob_stream_release(ctx);                       // first: joins the transcript threads of blob jobs still in flight (they may enqueue work until then)
    (void)hipStreamSynchronize(ctx->stream);
    for (auto st : ctx->stream_x) if (st) (void)hipStreamSynchronize(st);
    if (ctx->lag_stream) (void)hipStreamSynchronize(ctx->lag_stream);
    msm_drop_slots(ctx);
    ctx->last_sorted = nullptr; ctx->last_sorted_stream = nullptr;
    ctx->msm.release();
    for (auto& w : ctx->msm_x) w.release();
    for (auto& st : ctx->stream_x) if (st) { (void)hipStreamDestroy(st); st = nullptr; }
    ctx->ntt.release();
    for (auto& w : ctx->ntt_x) w.release();
    for (auto& ps : ctx->poly) ps.release();
    for (auto& b : ctx->mp) b.release();
    ctx->mp_ntt.release();
    for (auto& b : ctx->mv) b.release();
    for (auto& b : ctx->ml) b.release();
    for (auto& b : ctx->fs) b.release();
    for (auto& b : ctx->cb) b.release();
    ctx->mv_ntt.release();
    for (auto& b : ctx->rc) b.release();
    ctx->rc_ntt.release();
    for (auto& b : ctx->pc) b.release();
    ctx->pc_ntt.release();
    for (auto& b : ctx->pr) b.release();
    for (auto& b : ctx->pb) b.release();
    ctx->rccl_buf.release();
    if (ctx->rccl_pinned) { (void)hipHostFree(ctx->rccl_pinned); ctx->rccl_pinned = nullptr; ctx->rccl_pinned_bytes = 0; }
    if (ctx->vb_pinned) { (void)hipHostFree(ctx->vb_pinned); ctx->vb_pinned = nullptr; ctx->vb_pinned_bytes = 0; }
    for (auto& t : ctx->ondomain_inv) if (t) { (void)hipFree(t); t = nullptr; }
    for (auto& ev : ctx->lag_uploaded) if (ev) { (void)hipEventDestroy(ev); ev = nullptr; }
    for (auto& ev : ctx->lag_phase1) if (ev) { (void)hipEventDestroy(ev); ev = nullptr; }
    if (ctx->lag_stream) { (void)hipStreamSynchronize(ctx->lag_stream); (void)hipStreamDestroy(ctx->lag_stream); ctx->lag_stream = nullptr; }
    (void)hipStreamDestroy(ctx->stream);
    const int dev = ctx->device;
    delete ctx;
    // the caches are released UNDER the count mutex: a context created on this device meanwhile waits in kzg_ctx_create until they are gone
    // and then builds its own, instead of picking up pointers that are about to be freed
    std::lock_guard<std::mutex> lk(g_ctx_count_mu);
    const bool last = --g_ctx_count[dev] <= 0;
    if (last) { g_ctx_count.erase(dev); kzg::ntt_release_device_caches(dev); kzg::g1fft_release_device_caches(dev); }
}

const char* kzg_ctx_last_error(const kzg_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int32_t kzg_ctx_set_msm_window(kzg_ctx* ctx, int32_t c_bits, int32_t segment_len) {
    if (!ctx || c_bits < 0 || c_bits > 16 || c_bits == 1 || segment_len < 0) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->msm_c_override = c_bits;
    ctx->msm_seg_override = segment_len;
    return KZG_OK;
}

int32_t kzg_ctx_set_reduction_lanes(kzg_ctx* ctx, int32_t lanes) {
    if (!ctx || (lanes != 0 && lanes != 2 && lanes != 4)) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->reduction_lanes = lanes;
    return KZG_OK;
}

int32_t kzg_ctx_set_transcript_device(kzg_ctx* ctx, int32_t mode) {
    if (!ctx || mode < 0 || mode > 2) return KZG_ERR_INVALID_ARG;
    ctx->transcript_device.store(mode, std::memory_order_relaxed);
    return KZG_OK;
}

int32_t kzg_ctx_set_profiling(kzg_ctx* ctx, int32_t enable) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->profiling = enable != 0;
    for (int sl = 0; sl < KZG_NUM_SLOTS; ++sl) {
        MsmWorkspace& w = ctx->slot_msm(sl);
        for (auto& v : w.phase_ms) v = 0;
        w.profiled_launches = 0;
        w.profiled_pairs = 0;
        w.profiled_entries = 0;
    }
    return KZG_OK;
}

int32_t kzg_ctx_get_msm_profile(kzg_ctx* ctx, double phase_ms_out[8], uint64_t* launches, uint64_t* pairs) {
    if (!ctx || !phase_ms_out) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (int i = 0; i < 8; ++i) phase_ms_out[i] = 0;
    uint64_t nl = 0, np = 0;
    for (int sl = 0; sl < KZG_NUM_SLOTS; ++sl) {
        MsmWorkspace& w = ctx->slot_msm(sl);
        for (int i = 0; i < 8; ++i) phase_ms_out[i] += w.phase_ms[i];
        nl += w.profiled_launches;
        np += w.profiled_pairs;
    }
    if (launches) *launches = nl;
    if (pairs) *pairs = np;
    return KZG_OK;
}
int32_t kzg_ctx_get_msm_profile_entries(kzg_ctx* ctx, uint64_t* entries) {
    if (!ctx || !entries) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    uint64_t ne = 0;
    for (int sl = 0; sl < KZG_NUM_SLOTS; ++sl) ne += ctx->slot_msm(sl).profiled_entries;
    *entries = ne;
    return KZG_OK;
}

// ---- MSM ------------------------------------------------------------------------------------------
int32_t kzg_msm_g1(kzg_ctx* ctx, const uint64_t* bases_xy_mont, size_t n_bases, const uint64_t* scalars_mont, size_t n_scalars,
                   uint64_t out_xy_mont[8], uint8_t* out_is_infinity) {
    if (!ctx || !out_xy_mont) return KZG_ERR_INVALID_ARG;
    if (n_bases != n_scalars) return KZG_ERR_MSM_LENGTH_MISMATCH;
    if (n_bases && (!bases_xy_mont || !scalars_mont)) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n_bases == 0) { write_identity(out_xy_mont, out_is_infinity, nullptr); return KZG_OK; }
    KZG_HIP_TRY(ctx, ctx->msm.bases.reserve(n_bases * 64));
    int32_t rc = upload_points(ctx, bases_xy_mont, n_bases, ctx->msm.bases.as<uint4>(), ctx->msm.bases_wire);
    if (rc != KZG_OK) return rc;
    const void* d_scalars;
    rc = stage_scalars(ctx, scalars_mont, n_scalars, &d_scalars);
    if (rc != KZG_OK) return rc;
    MsmBases b;
    b.points = ctx->msm.bases.as<uint4>();
    return msm_run(ctx, b, d_scalars, n_bases, out_xy_mont, out_is_infinity, nullptr);
}

int32_t kzg_msm_g1_batch(kzg_ctx* ctx, const uint64_t* bases_xy_mont, const uint64_t* scalars_mont, size_t n, size_t batch,
                         uint64_t* out_xy_mont, uint8_t* out_is_infinity) {
    return msm_g1_batch_impl(ctx, bases_xy_mont, scalars_mont, n, batch, out_xy_mont, out_is_infinity, nullptr);
}

int32_t kzg_msm_g1_srs(kzg_ctx* ctx, const kzg_srs* srs, size_t offset, const uint64_t* scalars_mont, size_t n,
                       uint64_t out_xy_mont[8], uint8_t* out_is_infinity) {
    if (!out_xy_mont) return KZG_ERR_INVALID_ARG;
    return msm_srs_common(ctx, srs, offset, scalars_mont, false, n, out_xy_mont, out_is_infinity, nullptr);
}
int32_t kzg_msm_g1_srs_device(kzg_ctx* ctx, const kzg_srs* srs, size_t offset, const void* d_scalars_mont, size_t n,
                              uint64_t out_xy_mont[8], uint8_t* out_is_infinity) {
    if (!out_xy_mont) return KZG_ERR_INVALID_ARG;
    return msm_srs_common(ctx, srs, offset, d_scalars_mont, true, n, out_xy_mont, out_is_infinity, nullptr);
}
int32_t kzg_msm_g1_srs_partial_device(kzg_ctx* ctx, const kzg_srs* srs, size_t offset, const void* d_scalars_mont, size_t n,
                                      uint64_t out_xyzz_mont[16]) {
    if (!out_xyzz_mont) return KZG_ERR_INVALID_ARG;
    return msm_srs_common(ctx, srs, offset, d_scalars_mont, true, n, nullptr, nullptr, out_xyzz_mont);
}
int32_t kzg_msm_g1_srs_partial(kzg_ctx* ctx, const kzg_srs* srs, size_t offset, const uint64_t* scalars_mont, size_t n,
                               uint64_t out_xyzz_mont[16]) {
    if (!out_xyzz_mont) return KZG_ERR_INVALID_ARG;
    return msm_srs_common(ctx, srs, offset, scalars_mont, false, n, nullptr, nullptr, out_xyzz_mont);
}

int32_t kzg_msm_g1_srs_device_begin(kzg_ctx* ctx, const kzg_srs* srs, size_t offset, const void* d_scalars_mont, size_t n, int32_t slot) {
    if (!ctx || !srs || srs->ctx->device != ctx->device || !d_scalars_mont) return KZG_ERR_INVALID_ARG;
    if (offset > srs->n || n > srs->n - offset) return KZG_ERR_MSM_LENGTH_MISMATCH;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return msm_begin(ctx, slot, srs_bases(srs, offset, n, ctx->msm_c_override == 0), d_scalars_mont, n);
}
int32_t kzg_msm_g1_srs_begin(kzg_ctx* ctx, const kzg_srs* srs, size_t offset, const uint64_t* scalars_mont, size_t n, int32_t slot) {
    if (!ctx || !srs || srs->ctx->device != ctx->device || !scalars_mont || slot < 0 || slot >= KZG_NUM_SLOTS) return KZG_ERR_INVALID_ARG;
    if (offset > srs->n || n > srs->n - offset) return KZG_ERR_MSM_LENGTH_MISMATCH;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->slot_pending[slot]) return KZG_ERR_INVALID_ARG;
    // H2D copy on the slot's own stream into the slot's own staging buffer: it overlaps the other slot's kernels
    hipStream_t st = nullptr;
    { int32_t rc = msm_slot_stream(ctx, slot, &st); if (rc != KZG_OK) return rc; }
    MsmWorkspace& ws = ctx->slot_msm(slot);
    KZG_HIP_TRY(ctx, ws.scalars.reserve(n * 32 + 32));
    if (n) KZG_HIP_TRY(ctx, hipMemcpyAsync(ws.scalars.p, scalars_mont, n * 32, hipMemcpyHostToDevice, st));
    return msm_begin(ctx, slot, srs_bases(srs, offset, n, ctx->msm_c_override == 0), ws.scalars.p, n);
}
int32_t kzg_msm_g1_srs_end(kzg_ctx* ctx, int32_t slot, uint64_t* out_xy_mont, uint8_t* out_is_infinity, uint64_t* out_xyzz_mont) {
    if (!ctx || (!out_xy_mont && !out_xyzz_mont)) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return msm_end(ctx, slot, out_xy_mont, out_is_infinity, out_xyzz_mont);
}

// ---- one batched launch, asynchronous: `count` scalar sets (separate device buffers, n scalars each) against srs[offset .. offset + n)
size_t kzg_msm_batch_capacity(size_t n) { return kzg::msm_batch_capacity(n); }
int32_t kzg_msm_g1_srs_device_begin_batch(kzg_ctx* ctx, kzg_srs* srs, size_t offset, const void* const* d_scalars_mont, size_t n, size_t count, int32_t slot) {
    if (!ctx || !srs || srs->ctx->device != ctx->device || !d_scalars_mont) return KZG_ERR_INVALID_ARG;
    if (offset > srs->n || n > srs->n - offset) return KZG_ERR_MSM_LENGTH_MISMATCH;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint4* bits = srs_bits(srs);
    if (!bits) {
        int32_t rc = srs_build_bit_tables(ctx, srs, true);
        if (rc != KZG_OK) return rc;
        bits = srs_bits(srs);
        if (!bits) { ctx->last_error = "no per-bit tables for this SRS (memory, or KZG_NO_NAF)"; return KZG_ERR_INVALID_ARG; }
    }
    MsmBases b;
    b.points = bits + 4 * offset; b.table_stride = (uint32_t)srs->n; b.c = 7; b.W = 255; b.naf = true;
    return msm_begin_batch(ctx, slot, b, d_scalars_mont, n, count);
}
int32_t kzg_msm_g1_srs_end_batch(kzg_ctx* ctx, int32_t slot, size_t count, uint64_t* out_xy_mont, uint8_t* out_is_infinity, uint64_t* out_xyzz_mont) {
    if (!ctx || (!out_xy_mont && !out_xyzz_mont)) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return msm_end_batch(ctx, slot, count, out_xy_mont, out_is_infinity, out_xyzz_mont);
}

int32_t kzg_g1_fold_partials(const uint64_t* partials_xyzz_mont, size_t count, uint64_t out_xy_mont[8], uint8_t* out_is_infinity) {
    if (!out_xy_mont || (count && !partials_xyzz_mont)) return KZG_ERR_INVALID_ARG;
    kzg_host::Xyzz acc = kzg_host::xyzz_inf();
    for (size_t i = 0; i < count; ++i) {
        kzg_host::Xyzz p;
        memcpy(&p, partials_xyzz_mont + 16 * i, 128);
        acc = kzg_host::xyzz_add(acc, p);
    }
    kzg_host::xyzz_to_affine(acc, out_xy_mont, out_is_infinity);
    return KZG_OK;
}

// ---- NTT ------------------------------------------------------------------------------------------
int32_t kzg_fr_ntt_device(kzg_ctx* ctx, void* d_data_mont, size_t n, int32_t inverse) {
    if (!ctx || (!d_data_mont && n)) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int32_t rc = ntt_run(ctx, d_data_mont, n, inverse != 0);
    if (rc != KZG_OK) return rc;
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KZG_OK;
}

int32_t kzg_fr_ntt(kzg_ctx* ctx, uint64_t* data_mont, size_t n, int32_t inverse) {
    if (!ctx || (!data_mont && n)) return KZG_ERR_INVALID_ARG;
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_NOT_POWER_OF_TWO;
    if (n > ((size_t)1 << 28)) return KZG_ERR_DOMAIN;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    KZG_HIP_TRY(ctx, ctx->poly[0].a.reserve(n * 32));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->poly[0].a.p, data_mont, n * 32, hipMemcpyHostToDevice, ctx->stream));
    int32_t rc = ntt_run(ctx, ctx->poly[0].a.p, n, inverse != 0);
    if (rc != KZG_OK) return rc;
    KZG_HIP_TRY(ctx, hipMemcpyAsync(data_mont, ctx->poly[0].a.p, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KZG_OK;
}

// ---- KZG surface ------------------------------------------------------------------------------------
int32_t kzg_commit_coeff_form(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* coeffs_mont, size_t n,
                              uint64_t out_xy_mont[8], uint8_t* out_is_infinity) {
    if (!ctx || !srs || !out_xy_mont) return KZG_ERR_INVALID_ARG;
    if (n > srs->n) return KZG_ERR_POLY_LENGTH;                       // kzg.rs:112-116
    return msm_srs_common(ctx, srs, 0, coeffs_mont, false, n, out_xy_mont, out_is_infinity, nullptr);
}

int32_t kzg_commit_eval_form(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* evals_mont, size_t n,
                             uint64_t out_xy_mont[8], uint8_t* out_is_infinity) {
    if (!ctx || !srs || srs->ctx != ctx || !out_xy_mont || (n && !evals_mont)) return KZG_ERR_INVALID_ARG;
    if (n > srs->n) return KZG_ERR_SRS_CAPACITY_EXCEEDED;             // kzg.rs:89-94
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_NOT_POWER_OF_TWO; // kzg.rs:265-269 (g1_ifft)
    if (n > ((size_t)1 << 28)) return KZG_ERR_DOMAIN;
    std::lock_guard<std::mutex> lk(ctx->mu);                            // (taken BEFORE the cache is looked at: kzg_srs_drop_lagrange frees the basis under this lock)
    if (const kzg_srs* cached = srs_cached_lagrange(srs, n))            // the reference's literal form: MSM over the Lagrange basis (kzg.rs:98-100);
        return msm_srs_locked(ctx, cached, 0, evals_mont, false, n, out_xy_mont, out_is_infinity, nullptr);   // large ones in two parts, the second upload hidden
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    KZG_HIP_TRY(ctx, ctx->poly[0].a.reserve(n * 32));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->poly[0].a.p, evals_mont, n * 32, hipMemcpyHostToDevice, ctx->stream));
    int32_t rc = ntt_run(ctx, ctx->poly[0].a.p, n, true);               // coefficients = IFFT(evaluations)
    if (rc != KZG_OK) return rc;
    return msm_run(ctx, srs_bases(srs, 0, n, ctx->msm_c_override == 0), ctx->poly[0].a.p, n, out_xy_mont, out_is_infinity, nullptr);
}

int32_t kzg_commit_coeff_form_batch(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* coeffs_mont, size_t n, size_t count,
                                    uint64_t* out_xy_mont, uint8_t* out_is_infinity) {
    return commit_batch_common(ctx, srs, coeffs_mont, false, false, n, count, out_xy_mont, out_is_infinity);
}
int32_t kzg_commit_coeff_form_batch_device(kzg_ctx* ctx, kzg_srs* srs, const void* d_coeffs_mont, size_t n, size_t count,
                                           uint64_t* out_xy_mont, uint8_t* out_is_infinity) {
    return commit_batch_common(ctx, srs, d_coeffs_mont, true, false, n, count, out_xy_mont, out_is_infinity);
}
int32_t kzg_commit_eval_form_batch(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* evals_mont, size_t n, size_t count,
                                   uint64_t* out_xy_mont, uint8_t* out_is_infinity) {
    return commit_batch_common(ctx, srs, evals_mont, false, true, n, count, out_xy_mont, out_is_infinity);
}
int32_t kzg_commit_eval_form_batch_device(kzg_ctx* ctx, kzg_srs* srs, const void* d_evals_mont, size_t n, size_t count,
                                          uint64_t* out_xy_mont, uint8_t* out_is_infinity) {
    return commit_batch_common(ctx, srs, d_evals_mont, true, true, n, count, out_xy_mont, out_is_infinity);
}

// ---- multi-GPU forms: this rank's SRS shard holds the powers [shard_lo, shard_lo + len(srs_shard)) -----------------------
int32_t kzg_commit_eval_form_partial(kzg_ctx* ctx, const kzg_srs* srs_shard, size_t shard_lo, const uint64_t* evals_mont, size_t n,
                                     uint64_t out_xyzz_mont[16]) {
    if (!ctx || !srs_shard || srs_shard->ctx->device != ctx->device || !out_xyzz_mont || (n && !evals_mont)) return KZG_ERR_INVALID_ARG;
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_NOT_POWER_OF_TWO;
    if (n > ((size_t)1 << 28)) return KZG_ERR_DOMAIN;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    KZG_HIP_TRY(ctx, ctx->poly[0].a.reserve(n * 32));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->poly[0].a.p, evals_mont, n * 32, hipMemcpyHostToDevice, ctx->stream));
    int32_t rc = ntt_run(ctx, ctx->poly[0].a.p, n, true);               // every rank transforms the whole polynomial (32 B/element; not sharded)
    if (rc != KZG_OK) return rc;
    if (shard_lo >= n) { KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); memset(out_xyzz_mont, 0, 128); return KZG_OK; }
    const size_t len = std::min(srs_shard->n, n - shard_lo);
    return msm_run(ctx, srs_bases(srs_shard, 0, len, ctx->msm_c_override == 0), ctx->poly[0].a.as<uint4>() + 2 * shard_lo, len, nullptr, nullptr, out_xyzz_mont);
}

int32_t kzg_compute_proof_partial(kzg_ctx* ctx, const kzg_srs* srs_shard, size_t shard_lo, const uint64_t* evals_mont, size_t n,
                                  const uint64_t* roots_mont, size_t n_roots, const uint64_t z_mont[4],
                                  uint64_t out_xyzz_mont[16], uint64_t* out_y_mont) {
    (void)roots_mont;
    if (!ctx || !srs_shard || srs_shard->ctx != ctx || !out_xyzz_mont || !z_mont || (n && !evals_mont)) return KZG_ERR_INVALID_ARG;
    if (n != n_roots) return KZG_ERR_ROOTS_LENGTH;
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_INVALID_INPUT_LENGTH;
    if (n > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return proof_run(ctx, srs_shard, evals_mont, n, z_mont, nullptr, nullptr, out_y_mont, true, shard_lo, out_xyzz_mont);
}

// ---- config 4 sharded by evaluation index over the Lagrange basis (lagrange.hip) --------------------------------------------------
int32_t kzg_commit_eval_form_lagrange_partial(kzg_ctx* ctx, const kzg_srs* lagrange_shard, const uint64_t* evals_slice_mont, size_t len,
                                              uint64_t out_xyzz_mont[16]) {
    if (!ctx || !lagrange_shard || !out_xyzz_mont) return KZG_ERR_INVALID_ARG;
    if (len > lagrange_shard->n) return KZG_ERR_SRS_CAPACITY_EXCEEDED;              // kzg.rs:89-94
    return msm_srs_common(ctx, lagrange_shard, 0, evals_slice_mont, false, len, nullptr, nullptr, out_xyzz_mont);
}
int32_t kzg_commit_eval_form_lagrange_partial_device(kzg_ctx* ctx, const kzg_srs* lagrange_shard, const void* d_evals_slice_mont, size_t len,
                                                     uint64_t out_xyzz_mont[16]) {
    if (!ctx || !lagrange_shard || !out_xyzz_mont) return KZG_ERR_INVALID_ARG;
    if (len > lagrange_shard->n) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    return msm_srs_common(ctx, lagrange_shard, 0, d_evals_slice_mont, true, len, nullptr, nullptr, out_xyzz_mont);
}
int32_t kzg_compute_proof_lagrange_begin(kzg_ctx* ctx, const kzg_srs* lagrange_shard, size_t shard_lo, const uint64_t* evals_slice_mont,
                                         size_t len, size_t n, const uint64_t z_mont[4], int32_t slot) {
    return lagrange_begin_common(ctx, lagrange_shard, shard_lo, evals_slice_mont, false, len, n, z_mont, slot);
}
int32_t kzg_compute_proof_lagrange_begin_device(kzg_ctx* ctx, const kzg_srs* lagrange_shard, size_t shard_lo, const void* d_evals_slice_mont,
                                                size_t len, size_t n, const uint64_t z_mont[4], int32_t slot) {
    return lagrange_begin_common(ctx, lagrange_shard, shard_lo, d_evals_slice_mont, true, len, n, z_mont, slot);
}
int32_t kzg_commit_and_prove_lagrange_begin(kzg_ctx* ctx, const kzg_srs* lagrange_shard, size_t shard_lo, const uint64_t* evals_slice_mont, size_t len,
                                            size_t n, const uint64_t z_mont[4], int32_t commit_slot, int32_t proof_slot) {
    if (commit_slot < 0) return KZG_ERR_INVALID_ARG;
    return lagrange_begin_common(ctx, lagrange_shard, shard_lo, evals_slice_mont, false, len, n, z_mont, proof_slot, commit_slot);
}
int32_t kzg_commit_and_prove_lagrange_begin_device(kzg_ctx* ctx, const kzg_srs* lagrange_shard, size_t shard_lo, const void* d_evals_slice_mont, size_t len,
                                                   size_t n, const uint64_t z_mont[4], int32_t commit_slot, int32_t proof_slot) {
    if (commit_slot < 0) return KZG_ERR_INVALID_ARG;
    return lagrange_begin_common(ctx, lagrange_shard, shard_lo, d_evals_slice_mont, true, len, n, z_mont, proof_slot, commit_slot);
}
int32_t kzg_compute_proof_lagrange_partial_y(kzg_ctx* ctx, int32_t slot, uint64_t out_ypart_mont[8]) {
    if (!ctx || !out_ypart_mont) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return lag_partial_y(ctx, slot, out_ypart_mont);
}
int32_t kzg_compute_proof_lagrange_continue(kzg_ctx* ctx, int32_t slot, const uint64_t y_mont[4]) {
    if (!ctx || !y_mont) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return lag_continue(ctx, slot, y_mont);
}
int32_t kzg_compute_proof_lagrange_end(kzg_ctx* ctx, int32_t slot, uint64_t out_part[32]) {
    if (!ctx || !out_part) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return lag_end(ctx, slot, out_part, nullptr);
}
int32_t kzg_commit_and_prove_lagrange_end(kzg_ctx* ctx, int32_t slot, uint64_t out_commit_xyzz_mont[16], uint64_t out_part[32]) {
    if (!ctx || !out_part || !out_commit_xyzz_mont) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return lag_end(ctx, slot, out_part, out_commit_xyzz_mont);
}
int32_t kzg_compute_proof_lagrange_abort(kzg_ctx* ctx, int32_t slot) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    lag_abort(ctx, slot);
    return KZG_OK;
}
int32_t kzg_compute_quotient_eval_on_domain(kzg_ctx* ctx, const uint64_t z_mont[4], const uint64_t* evals_mont, size_t n, const uint64_t value_mont[4],
                                            uint64_t out_quotient_mont[4]) {
    if (!ctx || !z_mont || !evals_mont || !value_mont || !out_quotient_mont) return KZG_ERR_INVALID_ARG;
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_NOT_POWER_OF_TWO;
    if (n > ((size_t)1 << 28)) return KZG_ERR_DOMAIN;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return lag_quotient_eval_on_domain(ctx, z_mont, evals_mont, n, value_mont, out_quotient_mont);
}
int32_t kzg_lagrange_fold_y(const uint64_t* yparts_mont, size_t count, size_t n, const uint64_t z_mont[4], uint64_t out_y_mont[4]) {
    if (!z_mont || !out_y_mont || (count && !yparts_mont)) return KZG_ERR_INVALID_ARG;
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_INVALID_INPUT_LENGTH;
    if (n > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    return lag_fold_y(yparts_mont, count, n, z_mont, out_y_mont);
}
int32_t kzg_lagrange_fold_proof(const uint64_t* parts, size_t count, size_t n, const uint64_t z_mont[4], uint64_t out_xy_mont[8],
                                uint8_t* out_is_infinity) {
    if (!z_mont || !out_xy_mont || (count && !parts)) return KZG_ERR_INVALID_ARG;
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_INVALID_INPUT_LENGTH;
    if (n > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    return lag_fold_proof(parts, count, n, z_mont, out_xy_mont, out_is_infinity);
}

int32_t kzg_blob_to_fr(kzg_ctx* ctx, const uint8_t* blob_bytes, size_t len, uint64_t* out_mont, size_t cap, size_t* n_out) {
    if (!ctx || !n_out) return KZG_ERR_INVALID_ARG;
    const size_t n_elems = (len + 31) / 32;
    if (n_elems > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;                       // polynomial.rs:42-46
    const size_t n_padded = next_pow2(n_elems);                                   // next_power_of_two(0) == 1
    *n_out = n_padded;                                                               // size query: out == NULL
    if (!out_mont || cap < n_padded || (len && !blob_bytes)) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    void* d = nullptr;
    int32_t rc = blob_to_fr_run(ctx, blob_bytes, len, n_padded, &d);
    if (rc != KZG_OK) return rc;
    KZG_HIP_TRY(ctx, hipMemcpyAsync(out_mont, d, n_padded * 32, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KZG_OK;
}

int32_t kzg_commit_blob(kzg_ctx* ctx, const kzg_srs* srs, const uint8_t* blob_bytes, size_t len,
                        uint64_t out_xy_mont[8], uint8_t* out_is_infinity) {
    if (!ctx || !srs || srs->ctx->device != ctx->device || !out_xy_mont || (len && !blob_bytes)) return KZG_ERR_INVALID_ARG;
    const size_t n_elems = (len + 31) / 32;
    if (n_elems > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    const size_t n = next_pow2(n_elems);
    if (n > srs->n) return KZG_ERR_SRS_CAPACITY_EXCEEDED;                            // kzg.rs:89-94
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const kzg_srs* cached = srs_cached_lagrange(srs, n);
    {
        // over the cached Lagrange basis a large blob goes in TWO parts on two slots, as msm_srs_common does for scalars: bytes -> Fr and the MSM of the
        // first part run while this thread sits in the upload of the second (no IFFT ties the parts together)
        const bool idle = !ctx->slot_pending[0] && !ctx->slot_pending[1] && ctx->lag[0].phase == 0 && ctx->lag[1].phase == 0;
        if (cached && idle && n >= ((size_t)1 << 19) && n <= MSM_SPLIT_MAX && ctx->msm_c_override == 0 && srs_bits(cached)) {
            const size_t half = ((size_t)((double)n * (n >= ((size_t)1 << 20) ? 0.375 : 0.44)) + 255) / 256 * 256;
            const size_t e_lo[2] = {0, half}, e_n[2] = {half, n - half};
            int32_t rc = KZG_OK;
            int begun = 0;
            for (int h = 0; h < 2 && rc == KZG_OK; ++h) {
                hipStream_t st = nullptr;
                rc = msm_slot_stream(ctx, h, &st);
                if (rc != KZG_OK) break;
                MsmWorkspace& ws = ctx->slot_msm(h);
                const size_t b_lo = std::min(len, e_lo[h] * 32), b_hi = std::min(len, (e_lo[h] + e_n[h]) * 32);
                void* d_part = nullptr;
                rc = blob_to_fr_run(ctx, blob_bytes + b_lo, b_hi - b_lo, e_n[h], &d_part, st, &ws.blob, &ws.scalars);
                if (rc == KZG_OK) rc = msm_begin(ctx, h, srs_bases(cached, e_lo[h], e_n[h], true), d_part, e_n[h]);
                if (rc == KZG_OK) ++begun;
            }
            kzg_host::Xyzz parts[2] = {kzg_host::xyzz_inf(), kzg_host::xyzz_inf()};
            for (int h = 0; h < begun; ++h) {
                uint64_t w[16];
                const int32_t r2 = msm_end(ctx, h, nullptr, nullptr, w);
                if (r2 == KZG_OK) memcpy(&parts[h], w, 128); else if (rc == KZG_OK) rc = r2;
            }
            if (rc != KZG_OK) return rc;
            kzg_host::xyzz_to_affine(kzg_host::xyzz_add(parts[0], parts[1]), out_xy_mont, out_is_infinity);
            return KZG_OK;
        }
    }
    void* d = nullptr;
    int32_t rc = blob_to_fr_run(ctx, blob_bytes, len, n, &d);                        // Blob::to_polynomial_eval_form
    if (rc != KZG_OK) return rc;
    if (cached)                                                                      // commit_eval_form's literal form (kzg.rs:98-100): MSM over the cached Lagrange basis
        return msm_run(ctx, srs_bases(cached, 0, n, ctx->msm_c_override == 0), d, n, out_xy_mont, out_is_infinity, nullptr);
    rc = ntt_run(ctx, d, n, true);                                                   // commit_eval_form: IFFT ...
    if (rc != KZG_OK) return rc;
    return msm_run(ctx, srs_bases(srs, 0, n, ctx->msm_c_override == 0), d, n, out_xy_mont, out_is_infinity, nullptr);   // ... + MSM
}

int32_t kzg_commit_eval_form_begin(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* evals_mont, size_t n, int32_t slot) {
    if (!ctx || !srs || srs->ctx->device != ctx->device || !evals_mont) return KZG_ERR_INVALID_ARG;
    return commit_begin_common(ctx, srs, evals_mont, nullptr, 0, n, slot);
}
int32_t kzg_commit_blob_begin(kzg_ctx* ctx, const kzg_srs* srs, const uint8_t* blob_bytes, size_t len, int32_t slot) {
    if (!ctx || !srs || srs->ctx->device != ctx->device || (len && !blob_bytes)) return KZG_ERR_INVALID_ARG;
    const size_t n_elems = (len + 31) / 32;
    if (n_elems > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    return commit_begin_common(ctx, srs, nullptr, blob_bytes, len, next_pow2(n_elems), slot);
}

int32_t kzg_g1_ifft(kzg_ctx* ctx, const kzg_srs* srs, size_t n, uint64_t* out_xy_mont) {
    if (!ctx || !srs || srs->ctx != ctx) return KZG_ERR_INVALID_ARG;
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_NOT_POWER_OF_TWO;             // kzg.rs:265-269
    if (n > ((size_t)1 << 28)) return KZG_ERR_DOMAIN;                               // kzg.rs:275-278
    if (n > srs->n) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    if (!out_xy_mont) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return g1_ifft_run(ctx, srs, n, out_xy_mont);
}

int32_t kzg_compute_proof(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* evals_mont, size_t n,
                          const uint64_t* roots_mont, size_t n_roots, const uint64_t z_mont[4],
                          uint64_t out_xy_mont[8], uint8_t* out_is_infinity, uint64_t* out_y_mont) {
    (void)roots_mont;   // KZG::expanded_roots_of_unity can only hold the canonical domain (kzg.rs:65-72): its length is what is checked
    if (!ctx || !srs || srs->ctx != ctx || !out_xy_mont || !z_mont || (n && !evals_mont)) return KZG_ERR_INVALID_ARG;
    if (n != n_roots) return KZG_ERR_ROOTS_LENGTH;                    // kzg.rs:135-139, :222-226
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_INVALID_INPUT_LENGTH;
    if (n > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    if (n > srs->n) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return proof_run(ctx, srs, evals_mont, n, z_mont, out_xy_mont, out_is_infinity, out_y_mont, true, 0, nullptr);
}

int32_t kzg_compute_proof_begin(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* evals_mont, size_t n,
                                const uint64_t* roots_mont, size_t n_roots, const uint64_t z_mont[4], int32_t slot) {
    (void)roots_mont;
    if (!ctx || !srs || srs->ctx != ctx || !z_mont || (n && !evals_mont)) return KZG_ERR_INVALID_ARG;
    if (n != n_roots) return KZG_ERR_ROOTS_LENGTH;
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_INVALID_INPUT_LENGTH;
    if (n > ((size_t)1 << 24)) return KZG_ERR_TOO_LARGE;
    if (n > srs->n) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return proof_begin(ctx, srs, evals_mont, n, z_mont, slot);
}
int32_t kzg_compute_proof_end(kzg_ctx* ctx, int32_t slot, uint64_t out_xy_mont[8], uint8_t* out_is_infinity, uint64_t* out_y_mont) {
    if (!ctx || !out_xy_mont) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return proof_end(ctx, slot, out_xy_mont, out_is_infinity, out_y_mont);
}

// ---- Fiat-Shamir challenge and blob proofs (helpers.rs:411-472, kzg.rs:288-309) --------------------------------------------
int32_t kzg_validate_g1_point(const uint64_t xy_mont[8]) {
    if (!xy_mont) return KZG_ERR_INVALID_ARG;
    return kzg_host::g1_on_curve(kzg_host::g1_from_wire(xy_mont)) ? KZG_OK : KZG_ERR_G1_NOT_ON_CURVE;
}

int32_t kzg_hash_to_field_element(const uint8_t* msg, size_t len, uint64_t out_mont[4]) {
    if (!out_mont || (len && !msg)) return KZG_ERR_INVALID_ARG;
    using namespace kzg_host;
    Sha256 sh;
    sha256_init(sh);
    if (len) sha256_update(sh, msg, len);
    uint8_t dig[32];
    sha256_final(sh, dig);
    digest_to_fr_wire(dig, out_mont);
    return KZG_OK;
}

int32_t kzg_compute_challenge(const uint8_t* blob_bytes, size_t len, const uint64_t commitment_xy_mont[8], uint64_t out_z_mont[4]) {
    if (!commitment_xy_mont || !out_z_mont || (len && !blob_bytes)) return KZG_ERR_INVALID_ARG;
    if ((len + 31) / 32 > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    kzg_host::G1 c = kzg_host::g1_from_wire(commitment_xy_mont);
    if (!kzg_host::g1_on_curve(c)) return KZG_ERR_G1_NOT_ON_CURVE;                   // validate_g1_point (helpers.rs:694-708; cofactor 1)
    kzg_host::Sha256 sh;
    kzg_host::sha256_init(sh);
    challenge_absorb_prefix(sh, blob_bytes, len, blob_padded_len(len));
    challenge_finish(sh, c, out_z_mont);
    return KZG_OK;
}

int32_t kzg_compute_blob_proof(kzg_ctx* ctx, const kzg_srs* srs, const uint8_t* blob_bytes, size_t len, size_t n_roots,
                               const uint64_t commitment_xy_mont[8], uint64_t out_proof_xy_mont[8], uint8_t* out_is_infinity,
                               uint64_t* out_z_mont, uint64_t* out_y_mont) {
    if (!commitment_xy_mont) return KZG_ERR_INVALID_ARG;
    return blob_proof_common(ctx, srs, blob_bytes, len, n_roots, commitment_xy_mont, nullptr, nullptr, out_proof_xy_mont, out_is_infinity,
                             out_z_mont, out_y_mont);
}

int32_t kzg_commit_and_prove_blob(kzg_ctx* ctx, const kzg_srs* srs, const uint8_t* blob_bytes, size_t len, size_t n_roots,
                                  uint64_t out_commitment_xy_mont[8], uint8_t* out_commitment_is_infinity,
                                  uint64_t out_proof_xy_mont[8], uint8_t* out_proof_is_infinity, uint64_t* out_z_mont, uint64_t* out_y_mont) {
    if (!out_commitment_xy_mont) return KZG_ERR_INVALID_ARG;
    return blob_proof_common(ctx, srs, blob_bytes, len, n_roots, nullptr, out_commitment_xy_mont, out_commitment_is_infinity,
                             out_proof_xy_mont, out_proof_is_infinity, out_z_mont, out_y_mont);
}

int32_t kzg_evaluate_polynomial_in_evaluation_form(kzg_ctx* ctx, const uint64_t* evals_mont, size_t n,
                                                   const uint64_t z_mont[4], uint64_t out_y_mont[4]) {
    if (!ctx || !z_mont || !out_y_mont || (n && !evals_mont)) return KZG_ERR_INVALID_ARG;
    if (n == 0) return KZG_ERR_ZERO_LENGTH;
    if ((n & (n - 1)) != 0) return KZG_ERR_INVALID_INPUT_LENGTH;      // helpers.rs:485-487
    if (n > ((size_t)1 << 28)) return KZG_ERR_SRS_LENGTH;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return proof_run(ctx, nullptr, evals_mont, n, z_mont, nullptr, nullptr, out_y_mont, false, 0, nullptr);
}

int32_t kzg_calculate_roots_of_unity(kzg_ctx* ctx, uint64_t length_of_data_after_padding, uint64_t* out_mont, size_t cap, size_t* n_out) {
    if (!ctx || !n_out) return KZG_ERR_INVALID_ARG;
    if (length_of_data_after_padding == 0) return KZG_ERR_ZERO_LENGTH;                  // helpers.rs:554-558
    uint64_t elems = (length_of_data_after_padding + 31) / 32;
    if (elems > ((uint64_t)1 << 28)) return KZG_ERR_SRS_LENGTH;                          // helpers.rs:560-566
    const size_t n = next_pow2((size_t)elems);
    *n_out = n;
    if (!out_mont || cap < n) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return roots_run(ctx, out_mont, n);
}

}  // extern "C"

#if defined(KZG_DEVICE_BOUND_CHECK)
#include "field29.h"
KZG_BOUND_CHECK_EXPORTS(capi)
#endif
