// capi_g2.hip — the G2 part of the C-ABI (include/kzg_bn254_mi355x.h, "G2 on the device"): the device-resident G2 SRS handle, the G2
// MSM over caller bases or a handle, G2 commitments, the blob header (commitment, length commitment, length proof) in one call, its
// verification by two pairing checks, and the host decoder of gnark-compressed G2 points.  The kernels and their driver are
// g2msm.hip; every argument check here runs before any launch.
#include "engine.h"
#include <new>
#include "field29.h"
#include "host_g2_decode.h"

#include <atomic>
#include <string>
#include <vector>
#include <cstring>

using namespace kzg;

namespace {

bool is_pow2(uint64_t v) { return v != 0 && (v & (v - 1)) == 0; }

// the synchronous calls share slot 0's workspace and stream
bool slot0_busy(kzg_ctx* ctx) {
    if (!ctx->slot_pending[0]) return false;
    ctx->last_error = "a kzg_*_begin on slot 0 is still in flight: call kzg_msm_g1_srs_end(ctx, 0, ..) first";
    return true;
}
void write_g2_identity(uint64_t out[16], uint8_t* out_inf) {
    memset(out, 0, 128);
    if (out_inf) *out_inf = 1;
}
int32_t stage_scalars_g2(kzg_ctx* ctx, const uint64_t* scalars, size_t n, const void** d_out) {
    KZG_HIP_TRY(ctx, ctx->msm.scalars.reserve(n * 32 + 32));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->msm.scalars.p, scalars, n * 32, hipMemcpyHostToDevice, ctx->stream));
    *d_out = ctx->msm.scalars.p;
    return KZG_OK;
}
kzg_g2srs* new_handle(kzg_ctx* ctx, size_t n, int32_t* rc) {
    *rc = KZG_OK;
    kzg_g2srs* s = new (std::nothrow) kzg_g2srs();
    if (!s) { *rc = KZG_ERR_INVALID_ARG; return nullptr; }
    s->ctx = ctx;
    s->n = n;
    if (n) {
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->d_points), n * 128);
        if (e != hipSuccess) { delete s; *rc = set_error(ctx, e, "hipMalloc(g2 srs)"); return nullptr; }
    }
    return s;
}
void drop_handle(kzg_g2srs* s) {
    if (s->d_points) (void)hipFree(s->d_points);
    delete s;
}

// (the caller holds ctx->mu)
int32_t msm_g2_srs_locked(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, const void* scalars, bool on_device, size_t n,
                          uint64_t out[16], uint8_t* out_inf) {
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    if (n == 0) { write_g2_identity(out, out_inf); return KZG_OK; }
    const void* d_scalars = scalars;
    if (!on_device) { const int32_t rc = stage_scalars_g2(ctx, static_cast<const uint64_t*>(scalars), n, &d_scalars); if (rc != KZG_OK) return rc; }
    const uint4* pts[1] = {srs->d_points + 8 * offset};
    return g2_msm_run(ctx, pts, 1, d_scalars, n, out, out_inf);
}
int32_t msm_g2_srs_common(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, const void* scalars, bool on_device, size_t n,
                          uint64_t out[16], uint8_t* out_inf) {
    if (!ctx || !srs || srs->ctx->device != ctx->device || !out || (n && !scalars)) return KZG_ERR_INVALID_ARG;
    if (offset > srs->n || n > srs->n - offset) return KZG_ERR_POLY_LENGTH;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return msm_g2_srs_locked(ctx, srs, offset, scalars, on_device, n, out, out_inf);
}

}  // namespace

extern "C" {

int32_t kzg_g2srs_upload(kzg_ctx* ctx, const uint64_t* g2_mont, size_t n_points, kzg_g2srs** out, uint64_t* bad_index) {
    if (!ctx || !out || (n_points && !g2_mont)) return KZG_ERR_INVALID_ARG;
    *out = nullptr;
    if (n_points > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    int32_t rc;
    kzg_g2srs* s = new_handle(ctx, n_points, &rc);
    if (!s) return rc;
    int64_t bad = -1;
    rc = g2_upload_points(ctx, g2_mont, n_points, s->d_points, &bad);
    if (rc == KZG_OK && bad >= 0) {
        if (bad_index) *bad_index = (uint64_t)bad;
        rc = KZG_ERR_NOT_ON_CURVE;
    }
    if (rc != KZG_OK) { drop_handle(s); return rc; }
    *out = s;
    return KZG_OK;
}

int32_t kzg_g2srs_generate(kzg_ctx* ctx, const uint64_t tau_mont[4], uint64_t first_power, size_t n_points, kzg_g2srs** out) {
    if (!ctx || !out || !tau_mont) return KZG_ERR_INVALID_ARG;
    *out = nullptr;
    if (n_points > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    kzg_g2srs* s = new_handle(ctx, n_points, &rc);
    if (!s) return rc;
    rc = g2_generate_points(ctx, tau_mont, first_power, n_points, s->d_points);
    if (rc != KZG_OK) { drop_handle(s); return rc; }
    *out = s;
    return KZG_OK;
}

int32_t kzg_g2srs_download(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, size_t n, uint64_t* out_g2_mont) {
    if (!ctx || !srs || srs->ctx->device != ctx->device || (n && !out_g2_mont)) return KZG_ERR_INVALID_ARG;
    if (offset > srs->n || n > srs->n - offset) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    return g2_download_points(ctx, srs->d_points + 8 * offset, n, out_g2_mont);
}

size_t kzg_g2srs_len(const kzg_g2srs* srs) { return srs ? srs->n : 0; }

void kzg_g2srs_free(kzg_g2srs* srs) {
    if (!srs) return;
    if (srs->d_points) { (void)hipSetDevice(srs->ctx->device); (void)hipFree(srs->d_points); }
    delete srs;
}

int32_t kzg_msm_g2(kzg_ctx* ctx, const uint64_t* bases_g2_mont, size_t n_bases, const uint64_t* scalars_mont, size_t n_scalars,
                   uint64_t out_g2_mont[16], uint8_t* out_is_infinity) {
    if (!ctx || !out_g2_mont) return KZG_ERR_INVALID_ARG;
    if (n_bases != n_scalars) return KZG_ERR_MSM_LENGTH_MISMATCH;
    if (n_bases && (!bases_g2_mont || !scalars_mont)) return KZG_ERR_INVALID_ARG;
    if (n_bases > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    if (n_bases == 0) { write_g2_identity(out_g2_mont, out_is_infinity); return KZG_OK; }
    KZG_HIP_TRY(ctx, ctx->msm.bases.reserve(n_bases * 128));
    int64_t bad = -1;
    int32_t rc = g2_upload_points(ctx, bases_g2_mont, n_bases, ctx->msm.bases.as<uint4>(), &bad);
    if (rc != KZG_OK) return rc;
    if (bad >= 0) { ctx->last_error = "kzg_msm_g2: base " + std::to_string(bad) + " is not on the twist"; return KZG_ERR_NOT_ON_CURVE; }
    const void* d_scalars;
    rc = stage_scalars_g2(ctx, scalars_mont, n_scalars, &d_scalars);
    if (rc != KZG_OK) return rc;
    const uint4* pts[1] = {ctx->msm.bases.as<uint4>()};
    return g2_msm_run(ctx, pts, 1, d_scalars, n_bases, out_g2_mont, out_is_infinity);
}

int32_t kzg_msm_g2_srs(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, const uint64_t* scalars_mont, size_t n,
                       uint64_t out_g2_mont[16], uint8_t* out_is_infinity) {
    return msm_g2_srs_common(ctx, srs, offset, scalars_mont, false, n, out_g2_mont, out_is_infinity);
}
int32_t kzg_msm_g2_srs_device(kzg_ctx* ctx, const kzg_g2srs* srs, size_t offset, const void* d_scalars_mont, size_t n,
                              uint64_t out_g2_mont[16], uint8_t* out_is_infinity) {
    return msm_g2_srs_common(ctx, srs, offset, d_scalars_mont, true, n, out_g2_mont, out_is_infinity);
}

int32_t kzg_commit_g2_coeff_form(kzg_ctx* ctx, const kzg_g2srs* srs, const uint64_t* coeffs_mont, size_t n,
                                 uint64_t out_g2_mont[16], uint8_t* out_is_infinity) {
    return msm_g2_srs_common(ctx, srs, 0, coeffs_mont, false, n, out_g2_mont, out_is_infinity);       // n > len -> KZG_ERR_POLY_LENGTH
}

int32_t kzg_commit_g2_eval_form(kzg_ctx* ctx, const kzg_g2srs* srs, const uint64_t* evals_mont, size_t n,
                                uint64_t out_g2_mont[16], uint8_t* out_is_infinity) {
    if (!ctx || !srs || srs->ctx->device != ctx->device || !out_g2_mont || (n && !evals_mont)) return KZG_ERR_INVALID_ARG;
    if (n > srs->n) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    if (!is_pow2(n)) return KZG_ERR_NOT_POWER_OF_TWO;
    if (n > ((size_t)1 << 28)) return KZG_ERR_DOMAIN;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    KZG_HIP_TRY(ctx, ctx->poly[0].a.reserve(n * 32));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->poly[0].a.p, evals_mont, n * 32, hipMemcpyHostToDevice, ctx->stream));
    const int32_t rc = ntt_run(ctx, ctx->poly[0].a.p, n, true);          // coefficients = IFFT(evaluations)
    if (rc != KZG_OK) return rc;
    const uint4* pts[1] = {srs->d_points};
    return g2_msm_run(ctx, pts, 1, ctx->poly[0].a.p, n, out_g2_mont, out_is_infinity);
}

int32_t kzg_commit_with_length_proof(kzg_ctx* ctx, const kzg_srs* g1_srs, const kzg_g2srs* g2_srs, const kzg_g2srs* g2_trailing,
                                     uint64_t trailing_first_power, uint64_t srs_order, const uint64_t* coeffs_mont, size_t n,
                                     uint64_t claimed_len, uint64_t out_commitment_xy[8], uint64_t out_length_commitment[16],
                                     uint64_t out_length_proof[16]) {
    if (!ctx || !g1_srs || !g2_srs || !g2_trailing || !out_commitment_xy || !out_length_commitment || !out_length_proof || (n && !coeffs_mont))
        return KZG_ERR_INVALID_ARG;
    if (g1_srs->ctx->device != ctx->device || g2_srs->ctx->device != ctx->device || g2_trailing->ctx->device != ctx->device) return KZG_ERR_INVALID_ARG;
    if (!is_pow2(srs_order) || !is_pow2(claimed_len)) return KZG_ERR_NOT_POWER_OF_TWO;
    if (n > claimed_len || claimed_len > srs_order) return KZG_ERR_INVALID_ARG;
    // the proof's bases [tau^(N - d + i)]_2, i < n: from this offset of the trailing handle
    if (srs_order - claimed_len < trailing_first_power) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    const uint64_t off = srs_order - claimed_len - trailing_first_power;
    if (off > g2_trailing->n || claimed_len > g2_trailing->n - off) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    if (n > g1_srs->n || n > g2_srs->n) return KZG_ERR_POLY_LENGTH;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_busy(ctx)) return KZG_ERR_INVALID_ARG;
    if (n == 0) {
        memset(out_commitment_xy, 0, 64); memset(out_length_commitment, 0, 128); memset(out_length_proof, 0, 128);
        return KZG_OK;
    }
    const void* d_scalars;
    int32_t rc = stage_scalars_g2(ctx, coeffs_mont, n, &d_scalars);      // the one upload: all three MSMs read it
    if (rc != KZG_OK) return rc;
    rc = msm_srs_locked(ctx, g1_srs, 0, d_scalars, true, n, out_commitment_xy, nullptr, nullptr);
    if (rc != KZG_OK) return rc;
    const uint4* pts[2] = {g2_srs->d_points, g2_trailing->d_points + 8 * off};
    uint64_t out2[32];
    rc = g2_msm_run(ctx, pts, 2, d_scalars, n, out2, nullptr);           // one digit pass and sort, two accumulations
    if (rc != KZG_OK) return rc;
    memcpy(out_length_commitment, out2, 128);
    memcpy(out_length_proof, out2 + 16, 128);
    return KZG_OK;
}

int32_t kzg_verify_length_proof(const uint64_t commitment_xy[8], const uint64_t length_commitment[16], const uint64_t length_proof[16],
                                const uint64_t g1_tau_shift_xy[8], int32_t* out_ok) {
    if (!commitment_xy || !length_commitment || !length_proof || !g1_tau_shift_xy || !out_ok) return KZG_ERR_INVALID_ARG;
    using namespace kzg_host;
    const G1 c = g1_from_wire(commitment_xy), shift = g1_from_wire(g1_tau_shift_xy);
    const G2 c2 = g2_from_wire(length_commitment), pi2 = g2_from_wire(length_proof);
    if (!g1_on_curve(c) || !g1_on_curve(shift)) return KZG_ERR_G1_NOT_ON_CURVE;
    if (!g2_on_curve(c2) || !g2_on_curve(pi2)) return KZG_ERR_G2_TAU_NOT_ON_CURVE;
    G1 g1; g1.x = FQ_ONE; g1.y = FQ_TWO; g1.inf = false;
    const G2 g2 = g2_generator();
    // e(C, G2) = e(G1, C2): the two commitments hold the same polynomial; e([tau^(N-d)]_1, C2) = e(G1, pi2): pi2 is its shift by N - d
    *out_ok = pairings_verify(c, g2, g1, c2) && pairings_verify(shift, c2, g1, pi2) ? 1 : 0;
    return KZG_OK;
}

int32_t kzg_g2_decompress_be(const uint8_t* bytes, size_t n_points, uint64_t* out_g2_mont, uint64_t* bad_index) {
    if ((n_points && (!bytes || !out_g2_mont))) return KZG_ERR_INVALID_ARG;
    std::atomic<uint64_t> first_bad{UINT64_MAX};
    std::vector<int32_t> status(n_points, KZG_OK);
    host_parallel_for(n_points, [&](size_t i) {
        kzg_host::G2 p;
        status[i] = kzg_host::g2_decompress_be(bytes + 64 * i, p);
        if (status[i] == KZG_OK) { kzg_host::g2_to_wire(p, out_g2_mont + 16 * i); return; }
        uint64_t cur = first_bad.load();
        while (i < cur && !first_bad.compare_exchange_weak(cur, (uint64_t)i)) {}
    });
    const uint64_t bad = first_bad.load();
    if (bad == UINT64_MAX) return KZG_OK;
    if (bad_index) *bad_index = bad;
    return status[bad];
}

}  // extern "C"

KZG_BOUND_CHECK_EXPORTS(capi_g2)
