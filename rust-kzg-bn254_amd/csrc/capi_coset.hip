// capi_coset.hip — the coset-proof verifiers of the C-ABI (the proofs: kzg_compute_multiproofs): the weights of the batch transcript, the
// interpolation entry, the batch equation on wire words and on serialized bytes (two front ends, coset_stage_words and coset_stage_bytes, leave the items
// of a call on the device; one tail, coset_batch_tail, runs it), the retriever's call on top of the bytes front end (verify, then recover.hip on the
// value bytes the front end left on the device), the group sums and the search for the bad groups, and the three entries for batches of MIXED blob
// shapes (their own stage and tail: ragged values, a plan from host_coset_mixed.h, a product of several pairings).  Host scalars: host_coset_verify.h.
#include "engine.h"
#include "host_curve.h"
#include "host_fiat_shamir.h"
#include "host_coset_bytes.h"
#include "host_coset_verify.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

using namespace kzg;
using kzg_host::multiproof_r_powers_host;

namespace {

using kzg_host::coset_domain_check;   // the domain / chunk table of kzg_compute_multiproofs, in the documented order (host_coset_mixed.h: the mixed checks run it per class)

// the upload alone: values -> ctx->mv[0], weights | indices -> ctx->mv[1] (weights == nullptr: their place is left for the caller to fill on the
// device; ys == nullptr: room only); room for the l coefficients in ctx->mv[2].  Enqueued on ctx->stream; the caller holds ctx->mu
int32_t coset_upload(kzg_ctx* ctx, const uint64_t* ys, const uint64_t* coset_indices, const uint64_t* weights, size_t count, size_t l, uint4** d_w, uint64_t** d_k) {
    KZG_HIP_TRY(ctx, ctx->mv[0].reserve(std::max<size_t>(count * l * 32, 32)));           // (count == 0: the kernels still get valid pointers)
    KZG_HIP_TRY(ctx, ctx->mv[1].reserve(std::max<size_t>(count * 40, 64)));
    KZG_HIP_TRY(ctx, ctx->mv[2].reserve(l * 32));
    *d_w = ctx->mv[1].as<uint4>();
    *d_k = reinterpret_cast<uint64_t*>(ctx->mv[1].as<uint8_t>() + count * 32);
    if (count && ys) {
        KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->mv[0].p, ys, count * l * 32, hipMemcpyHostToDevice, ctx->stream));
        if (weights) KZG_HIP_TRY(ctx, hipMemcpyAsync(*d_w, weights, count * 32, hipMemcpyHostToDevice, ctx->stream));
        KZG_HIP_TRY(ctx, hipMemcpyAsync(*d_k, coset_indices, count * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    return KZG_OK;
}

// The host checks of kzg_verify_multiproof_batch, in the documented order.  grouped: the entries that take a partition of the items
// (kzg_coset_group_sums, kzg_verify_multiproof_batch_locate) add the checks of host_locate.h where their table puts them.
int32_t multiproof_batch_checks(const kzg_ctx* ctx, const kzg_srs* srs, bool output_null, bool input_null, bool g2_missing, size_t n_commitments,
                                const uint64_t* commitment_indices, const uint64_t* coset_indices, size_t count, size_t n, size_t chunk_len,
                                const uint64_t* group_indices, size_t n_groups, bool grouped) {
    if (!ctx || !srs || output_null) return KZG_ERR_INVALID_ARG;
    if (count && input_null) return KZG_ERR_INVALID_ARG;
    if (g2_missing) return KZG_ERR_INVALID_ARG;                                          // consts::G2_TAU is [tau]_2 only
    if (srs->ctx != ctx || srs->lagrange_of != 0) return KZG_ERR_INVALID_ARG;
    int32_t rc = coset_domain_check(n, chunk_len);
    if (rc != KZG_OK) return rc;
    const size_t l = chunk_len, m = n / l;
    if (l > srs->n) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    for (size_t i = 0; i < count; ++i) if (coset_indices[i] >= m || commitment_indices[i] >= n_commitments) return KZG_ERR_INVALID_ARG;
    if (grouped) { rc = locate_check_groups(group_indices, count, n_groups); if (rc != KZG_OK) return rc; }
    if (count > ((size_t)1 << 28) / l) return KZG_ERR_TOO_LARGE;
    if (grouped && n_groups > LOCATE_MAX_GROUPS) return KZG_ERR_TOO_LARGE;
    return KZG_OK;
}

// ---- the batch equation: two front ends, one tail -----------------------------------------------------------------------------------------
// Where the items of one call lie once a front end has run: N items on M commitment rows, cosets of l points of a domain of n.
struct CosetStage {
    std::unique_lock<std::mutex> lk;             // ctx->mu: taken by the front end, held until the entry is done with the device
    size_t N = 0, M = 0, n = 0, l = 0;
    const uint64_t *coset_indices = nullptr, *commitment_indices = nullptr;   // host, the caller's
    const uint64_t* r_powers = nullptr;          // host: the weights, supplied or derived (then in `derived`)
    std::vector<uint64_t> derived;
    uint4* d_ys = nullptr;                       // ctx->mv[0]: N x l wire values
    uint4* d_w = nullptr; uint64_t* d_k = nullptr;   // ctx->mv[1]: N wire weights | N coset indices
    uint4* d_bases = nullptr;                    // ctx->msm.bases, device format: proofs | proofs | commitments (the front ends of the batch equation)
    const char* rp_path = "";                    // trace: where the weights came from, and the front end's phase times
    double ms[3] = {0, 0, 0};
    // the shape and the host arrays; r == nullptr: room for the weights to derive.  Returns whether the device derives them (mode: kzg_ctx_set_transcript_device)
    bool begin(int mode, size_t N_, size_t M_, size_t n_, size_t l_, const uint64_t* ks, const uint64_t* rows, const uint64_t* r) {
        N = N_; M = M_; n = n_; l = l_;
        coset_indices = ks; commitment_indices = rows;
        if (!r) derived.resize(4 * N);
        r_powers = r ? r : derived.data();
        return !r && kzg_host::coset_transcript_on_device(mode, N, l);
    }
};

// N proofs -> d_proofs, M commitments -> d_commitments (device format), every point checked on the curve on its way; synchronised on return
int32_t coset_upload_points(kzg_ctx* ctx, const uint64_t* proofs, size_t N, const uint64_t* commitments, size_t M, uint4* d_proofs, uint4* d_commitments) {
    uint32_t off_p = 0, off_c = 0;
    int32_t rc = upload_points(ctx, proofs, N, d_proofs, ctx->msm.bases_wire, &off_p);
    if (rc == KZG_OK && M) rc = upload_points(ctx, commitments, M, d_commitments, ctx->msm.bases_wire, &off_c);
    if (rc != KZG_OK) return rc;
    return off_p || off_c ? KZG_ERR_G1_NOT_ON_CURVE : KZG_OK;
}

// The front end for wire words.  The weights: supplied, or derived on the host pool BEFORE ctx->mu is taken (threads that share a context overlap
// there; the host transcript never waits for the context), or on the device once the values have landed (mode: kzg_ctx_set_transcript_device, default the context's).
// Values, indices and weights go up once.  with_bases (the batch equation): the points go into the layout of CosetStage through the validating
// upload.  ms: r_powers, uploads.
int32_t coset_stage_words(kzg_ctx* ctx, const uint64_t* commitments, size_t M, const uint64_t* commitment_indices, const uint64_t* coset_indices, const uint64_t* ys,
                          const uint64_t* proofs, size_t N, size_t n, size_t l, const uint64_t* r_powers, bool with_bases, CosetStage* s, int mode = -1) {
    const bool trace = opts().vb_trace != 0;
    const auto t0 = Clock::now();
    const bool derive = !r_powers, on_device = s->begin(mode < 0 ? ctx->transcript_device.load(std::memory_order_relaxed) : mode, N, M, n, l, coset_indices, commitment_indices, r_powers);
    if (derive && !on_device) {
        RoctxRange range("kzg:multiproof_verify:r_powers (host)");
        multiproof_r_powers_host(commitments, M, commitment_indices, coset_indices, ys, proofs, N, n, l, s->derived.data(), host_parallel_for);
        s->rp_path = " (host)";
    }
    const auto t_host = Clock::now();
    s->lk = std::unique_lock<std::mutex>(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (with_bases && slot0_refused(ctx, true)) return KZG_ERR_INVALID_ARG;               // (the group sums meet their refusal later, behind the off-curve points)
    int32_t rc = coset_upload(ctx, ys, coset_indices, on_device ? nullptr : s->r_powers, N, l, &s->d_w, &s->d_k);
    if (rc != KZG_OK) return rc;
    s->d_ys = ctx->mv[0].as<uint4>();
    auto t_up = t_host;
    if (trace) { KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); t_up = Clock::now(); }
    if (on_device) {
        // the item digests are hashed where the values landed, the batch hash runs here, the weights are written where the interpolation reads them and
        // come back for the host scalars.  Inputs that are not canonical give the host's bits: that transcript is recomputed there and its weights uploaded
        bool fell_back = false;
        rc = coset_r_powers_device(ctx, commitments, M, commitment_indices, s->d_ys, s->d_k, proofs, N, n, l, s->d_w, s->derived.data(), &fell_back);
        if (rc != KZG_OK) return rc;
        if (fell_back) {
            multiproof_r_powers_host(commitments, M, commitment_indices, coset_indices, ys, proofs, N, n, l, s->derived.data(), host_parallel_for);
            KZG_HIP_TRY(ctx, hipMemcpyAsync(s->d_w, s->derived.data(), N * 32, hipMemcpyHostToDevice, ctx->stream));
            KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        s->rp_path = fell_back ? " (device, then host: an input is not canonical)" : " (device)";
    }
    const auto t_weights = Clock::now();
    if (with_bases) {
        KZG_HIP_TRY(ctx, ctx->msm.bases.reserve((2 * N + M) * 64));
        s->d_bases = ctx->msm.bases.as<uint4>();
        std::vector<uint64_t> twice(2 * N * 8);                                         // (one upload of 2 N points: a device copy of the first N costs a small
        memcpy(twice.data(), proofs, N * 64);                                           // batch more than it saves, profiles/coset_pipeline.md)
        memcpy(twice.data() + N * 8, proofs, N * 64);
        rc = coset_upload_points(ctx, twice.data(), 2 * N, commitments, M, s->d_bases, s->d_bases + 4 * 2 * N);
        if (rc != KZG_OK) return rc;
    }
    s->ms[0] = on_device ? ms_between(t_up, t_weights) : ms_between(t0, t_host);
    s->ms[1] = ms_between(t_host, t_up) + ms_between(t_weights, Clock::now());
    return KZG_OK;
}

// The front end for serialized bytes.  Values go up once as bytes (ctx->cb[0]) and are decoded where the interpolation kernel reads them; proofs
// and commitments go up as 32 bytes each (ctx->cb[1]) and are decoded straight into the layout of CosetStage (the decode kernel writes the
// second copy of the proofs).  Nothing decoded returns to the host.  The transcript reads the bytes: on the host pool beside the decode kernels,
// or on the device where the bytes landed.  who: the entry, for the line of a refused element.  ms: host r_powers beside the decode, decode, r_powers.
// item_status (kzg_retrieve_blobs_bytes_tolerant): a proof or value that does not decode does not end the call; item i gets its RETRIEVE_ITEM_* there
// (2 / 3 / 4, the smallest that applies, else 0), its decoded proof and values are zeros and its weight is ZERO wherever the stage keeps weights
// (s->r_powers, then a copy in s->derived, and s->d_w): the item enters every sum with weight 0 and every other item keeps its weight.  The
// transcript hashes the bytes as given on either path (host_fiat_shamir.h, fsdevice.hip: nothing there decodes), so a refusal changes no weight.
int32_t coset_stage_bytes(kzg_ctx* ctx, const char* who, const uint8_t* commitments_be, size_t M, const uint64_t* commitment_indices, const uint64_t* coset_indices,
                          const uint8_t* ys_be, const uint8_t* proofs_be, size_t N, size_t n, size_t l, const uint64_t* r_powers, bool g2_ok, uint64_t* bad_index,
                          int32_t* bad_array, CosetStage* s, std::vector<uint8_t>* item_status = nullptr) {
    const auto t0 = Clock::now();
    const bool derive = !r_powers, on_device = s->begin(ctx->transcript_device.load(std::memory_order_relaxed), N, M, n, l, coset_indices, commitment_indices, r_powers);
    s->lk = std::unique_lock<std::mutex>(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_refused(ctx)) return KZG_ERR_INVALID_ARG;
    // 0. uploads and decode kernels: everything is enqueued, then the host transcript runs beside them
    KZG_HIP_TRY(ctx, ctx->msm.bases.reserve((2 * N + M) * 64));
    int32_t rc = coset_upload(ctx, nullptr, nullptr, nullptr, N, l, &s->d_w, &s->d_k);
    if (rc != KZG_OK) return rc;
    s->d_bases = ctx->msm.bases.as<uint4>();
    s->d_ys = ctx->mv[0].as<uint4>();
    CosetBytesDecode job;
    job.points_be[0] = commitments_be; job.n_points[0] = M; job.d_points[0] = s->d_bases + 4 * 2 * N;
    job.points_be[1] = proofs_be; job.n_points[1] = N; job.d_points[1] = s->d_bases; job.d_points_copy[1] = s->d_bases + 4 * N;
    job.ys_be = ys_be; job.n_values = N * l; job.d_ys = s->d_ys;
    job.item_status = item_status != nullptr; job.values_per_item = l;
    rc = coset_bytes_enqueue(ctx, &job);
    if (rc != KZG_OK) return rc;
    hipError_t e_k = hipMemcpyAsync(s->d_k, coset_indices, N * 8, hipMemcpyHostToDevice, ctx->stream);
    if (derive && !on_device && e_k == hipSuccess) {
        RoctxRange range("kzg:multiproof_verify:r_powers (host, from bytes)");
        kzg_host::multiproof_r_powers_bytes_host(commitments_be, M, commitment_indices, coset_indices, ys_be, proofs_be, N, n, l, s->derived.data(), host_parallel_for);
    }
    const auto t_rp_host = Clock::now();
    rc = coset_bytes_collect(ctx, &job);                                                 // (drains the stream on every path: the copy of the indices too)
    if (e_k != hipSuccess) return set_error(ctx, e_k, "uploading the coset indices");
    if (rc != KZG_OK) return rc;
    static const char* const names[3] = {"commitment", "proof", "value of item"};
    for (int a = 0; a < 3; ++a) {
        rc = coset_bytes_status(ctx, who, names[a], job.bad[a], a == 2 ? l : 1, bad_index);
        if (rc != KZG_OK) { if (bad_array) *bad_array = a; return rc; }
    }
    if (!g2_ok) return KZG_ERR_G2_TAU_NOT_ON_CURVE;                                      // (before the device transcript, which nothing refuses)
    bool refused = false;
    if (item_status) {
        item_status->resize(N);
        for (size_t i = 0; i < N; ++i) {
            const uint32_t w = job.status[i];
            (*item_status)[i] = w & COSET_ITEM_PROOF_BYTES ? RETRIEVE_ITEM_PROOF_BYTES : w & COSET_ITEM_PROOF_OFF_CURVE ? RETRIEVE_ITEM_PROOF_OFF_CURVE
                                : w & COSET_ITEM_VALUE ? RETRIEVE_ITEM_VALUE : RETRIEVE_ITEM_GOOD;
            refused = refused || w != 0;
        }
    }
    auto mask_host = [&]() {                                                             // the host's copy of the weights, refused items zeroed
        if (!refused) return;
        if (s->r_powers != s->derived.data()) { s->derived.assign(s->r_powers, s->r_powers + 4 * N); s->r_powers = s->derived.data(); }
        for (size_t i = 0; i < N; ++i) if (job.status[i]) memset(s->derived.data() + 4 * i, 0, 32);
    };
    const auto t_dec = Clock::now();
    // 1. the weights where the interpolation reads them
    s->rp_path = derive ? " (host, from bytes, beside the decode)" : " (supplied)";
    if (on_device) {
        rc = coset_r_powers_device_bytes(ctx, commitments_be, M, commitment_indices, job.d_ys_be, s->d_k, job.d_points_be[1], N, n, l, s->d_w, s->derived.data());
        if (rc != KZG_OK) return rc;
        s->rp_path = " (device, from bytes)";
        mask_host();
        if (refused) { rc = coset_mask_refused_weights(ctx, s->d_w, job.d_status, N); if (rc != KZG_OK) return rc; }
    } else {
        mask_host();
        KZG_HIP_TRY(ctx, hipMemcpyAsync(s->d_w, s->r_powers, N * 32, hipMemcpyHostToDevice, ctx->stream));
    }
    s->ms[0] = derive && !on_device ? ms_between(t0, t_rp_host) : 0.0;
    s->ms[1] = ms_between(t0, t_dec);
    s->ms[2] = ms_between(t_dec, Clock::now());
    return KZG_OK;
}

// The tail: accept <=> e(sum_i r_i pi_i, [tau^l]_2) = e(sum_rows R_row C_row - sum_t A_t [tau^t]_1 + sum_i r_i w^(k_i l) pi_i, G2), from
// pi_i tau^l = C - I_i(tau) + w^(k_i l) pi_i.  For l = 1 this is batch.rs:228-254.  The caller holds the stage's lock; synchronised on return.
struct CosetTailTimes { Clock::time_point start, interpolated, coeff_msm, point_msms; };
int32_t coset_batch_tail(kzg_ctx* ctx, const kzg_srs* srs, const CosetStage& s, const kzg_host::G2& g2_tau_l, int32_t* out_ok, CosetTailTimes* t) {
    using namespace kzg_host;
    const size_t N = s.N, M = s.M, l = s.l;
    t->start = Clock::now();
    // 1. values, indices, weights -> the l coefficients A_t (left on the device)
    int32_t rc = coset_interpolate_rlc_device(ctx, s.d_ys, s.d_k, s.d_w, N, s.n, l, ctx->mv[2].as<uint4>());
    if (rc != KZG_OK) return rc;
    if (opts().vb_trace) KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    t->interpolated = Clock::now();
    // 2. [sum_i r_i I_i(tau)]_1: an MSM of the coefficients over srs[0 .. l)
    uint64_t interp_xy[8];
    uint8_t interp_inf = 0;
    rc = msm_srs_locked(ctx, srs, 0, ctx->mv[2].p, true, l, interp_xy, &interp_inf, nullptr);
    if (rc != KZG_OK) return rc;
    t->coeff_msm = Clock::now();
    // 3. host scalars: r_i | r_i w^(k_i l) | the row sums of the weights, in the order of the bases
    std::vector<uint64_t> scalars((2 * N + M) * 4);
    coset_batch_scalars(s.coset_indices, s.commitment_indices, s.r_powers, N, M, s.n / l, scalars.data(), host_parallel_for);
    // 4. the two N-point combinations of the proofs and the M-point one of the commitments
    KZG_HIP_TRY(ctx, ctx->msm.scalars.reserve((2 * N + M) * 32 + 32));
    const uint4* d_scalars = ctx->msm.scalars.as<uint4>();
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->msm.scalars.p, scalars.data(), (2 * N + M) * 32, hipMemcpyHostToDevice, ctx->stream));
    uint64_t sums[2 * 8], c_sum[8];
    uint8_t infs[2], c_inf = 0;
    rc = msm_run_batch(ctx, s.d_bases, d_scalars, N, 2, sums, infs);
    if (rc == KZG_OK) rc = msm_run_batch(ctx, s.d_bases + 4 * 2 * N, d_scalars + 2 * 2 * N, M, 1, c_sum, &c_inf);
    if (rc != KZG_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }            // (`scalars` is in use until the stream is drained)
    t->point_msms = Clock::now();
    // 5. point sums and ONE pairing check
    const G1 lhs = g1_from_wire(sums);
    const G1 rhs = g1_add(g1_add(g1_from_wire(c_sum), g1_neg(g1_from_wire(interp_xy))), g1_from_wire(sums + 8));
    *out_ok = pairings_verify_pooled(lhs, g2_tau_l, rhs, g2_generator()) ? 1 : 0;
    return KZG_OK;
}

// ---- the group sums of a batch of coset proofs (multilocate.hip, host_locate.h) -----------------------------------------------------------
struct GroupSums {
    LocatePlan plan;
    std::vector<kzg_host::Xyzz> lhs, rhs;        // per NON-EMPTY group (plan.segs): L_g, R_g
};

// The arguments have passed multiproof_batch_checks(.., grouped); count > 0.  Values, indices and weights go up once, in the caller's
// order; the kernels read through the plan's permutation.  Off-curve points are reported as the batch entry reports them.
int32_t coset_group_sums_core(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* commitments_xy_mont, size_t n_commitments, const uint64_t* commitment_indices,
                              const uint64_t* coset_indices, const uint64_t* ys_mont, const uint64_t* proofs_xy_mont, size_t N, size_t n, size_t l,
                              const uint64_t* r_powers_mont, const uint64_t* group_indices, size_t n_groups, GroupSums* out) {
    using namespace kzg_host;
    const auto t0 = Clock::now();
    int32_t rc = locate_plan(group_indices, N, n_groups, &out->plan);
    if (rc != KZG_OK) return rc;
    const LocatePlan& plan = out->plan;
    const size_t S = plan.segs.size(), M = n_commitments;
    CosetStage st;
    rc = coset_stage_words(ctx, commitments_xy_mont, M, commitment_indices, coset_indices, ys_mont, proofs_xy_mont, N, n, l, r_powers_mont, false, &st);
    if (rc != KZG_OK) return rc;
    // the points, validated on the device on their way into its format: N proofs, then the M commitments
    KZG_HIP_TRY(ctx, ctx->ml[5].reserve((N + M) * 64));
    rc = coset_upload_points(ctx, proofs_xy_mont, N, commitments_xy_mont, M, ctx->ml[5].as<uint4>(), ctx->ml[5].as<uint4>() + 4 * N);
    if (rc != KZG_OK) return rc;
    const auto t_up = Clock::now();                                                      // (upload_points synchronises)
    // 1. the plan, then the coefficients A_{g,t} of every non-empty group (left on the device)
    rc = locate_upload_plan(ctx, plan);
    if (rc != KZG_OK) return rc;
    rc = coset_group_coeffs_device(ctx, st.d_ys, st.d_k, st.d_w, plan, n, l);
    if (rc != KZG_OK) return rc;
    // 2. host scalars r_i w^(k_i l) beside those kernels; they and the commitment rows go up for the point sums
    std::vector<uint64_t> shifted(4 * N);
    coset_shifted_weights(coset_indices, st.r_powers, N, n / l, shifted.data(), host_parallel_for);
    KZG_HIP_TRY(ctx, ctx->ml[4].reserve(N * 40));
    uint4* d_w2 = ctx->ml[4].as<uint4>();
    uint64_t* d_ci = reinterpret_cast<uint64_t*>(ctx->ml[4].as<uint8_t>() + N * 32);
    KZG_HIP_TRY(ctx, hipMemcpyAsync(d_w2, shifted.data(), N * 32, hipMemcpyHostToDevice, ctx->stream));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(d_ci, commitment_indices, N * 8, hipMemcpyHostToDevice, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                                 // the MSM launches run on the slots' streams
    const auto t_interp = Clock::now();
    // 3. [sum_t A_{g,t} tau^t]_1 for every non-empty group: S polynomials of l coefficients as one MSM problem
    std::vector<uint64_t> interp_xy(8 * S);
    rc = commit_batch_device(ctx, srs, ctx->ml[0].p, l, S, interp_xy.data(), nullptr);
    if (rc != KZG_OK) return rc;
    const auto t_msm = Clock::now();
    // 4. the segmented point sums
    std::vector<uint64_t> sums(32 * S);
    rc = locate_point_sums_device(ctx, ctx->ml[5].as<uint4>(), d_ci, st.d_w, d_w2, plan, sums.data());
    if (rc != KZG_OK) return rc;
    st.lk.unlock();
    const auto t_pts = Clock::now();
    // 5. R_g = (point sum) - (interpolation commitment)
    out->lhs.resize(S);
    out->rhs.resize(S);
    const size_t per = 256;
    host_parallel_for((S + per - 1) / per, [&](size_t c) {
        for (size_t j = c * per; j < std::min(S, (c + 1) * per); ++j) {
            Xyzz b;
            memcpy(&out->lhs[j], sums.data() + 32 * j, 128);
            memcpy(&b, sums.data() + 32 * j + 16, 128);
            Xyzz i = xyzz_from_affine_wire(interp_xy.data() + 8 * j);
            i.y = neg(i.y);
            out->rhs[j] = xyzz_add(b, i);
        }
    });
    if (opts().vb_trace)
        fprintf(stderr, "coset_group_sums N=%zu l=%zu M=%zu groups=%zu (non-empty %zu): plan + r_powers + upload %.3f ms, interpolation + segment sums %.3f ms, "
                "coefficient MSMs %.3f ms, point sums %.3f ms, host sums %.3f ms\n", N, l, M, n_groups, S, ms_between(t0, t_up), ms_between(t_up, t_interp),
                ms_between(t_interp, t_msm), ms_between(t_msm, t_pts), ms_between(t_pts, Clock::now()));
    return KZG_OK;
}

// ---- the same sums over a stage that a bytes front end has left on the device (kzg_verify_multiproof_batch_locate_bytes, the tolerant retriever) ----
// What the stage holds and what survives a REJECTED coset_batch_tail over it (read from the code that runs there):
//   * the points, s.d_bases = proofs | proofs | commitments: every MSM driver takes its bases as const and sorts digits into its own workspace
//     (msm.hip: ws.sorted / ws.offs / buckets); nothing reserves or writes ctx->msm.bases behind the front end.  The point sums read the second
//     copy of the proofs and the commitments behind it, the layout locate_point_sums_device wants;
//   * the weights and coset indices, s.d_w / s.d_k in ctx->mv[1]: only read;
//   * the values, s.d_ys in ctx->mv[0]: read in place for l <= 1024; for l > 1024 the tail has replaced row i by IFFT_l(ys_i) (one ntt_run per
//     coset, the call coset_item_rows_device would make itself), so the rows are taken from there: `transformed`;
//   * the value bytes, ctx->cb[0], and the point bytes and status words, ctx->cb[1]: written by the front end only.
// The item rows are computed ONCE per call (ResidentSums::rows_ready) and summed under as many plans as the caller searches.
struct ResidentSums {
    const CosetStage* s = nullptr;
    bool transformed = false;                    // a tail has run over the stage (matters for l > 1024)
    bool rows_ready = false;
    uint4* d_w2 = nullptr; uint64_t* d_ci = nullptr;     // ctx->ml[4]: r_i w^(k_i l) | commitment rows, per item
};

int32_t resident_group_sums(kzg_ctx* ctx, kzg_srs* srs, ResidentSums* r, const LocatePlan& plan, GroupSums* out) {
    using namespace kzg_host;
    const CosetStage& st = *r->s;
    const size_t N = st.N, l = st.l, S = plan.segs.size();
    int32_t rc = KZG_OK;
    if (!r->rows_ready) {
        std::vector<uint64_t> shifted(4 * N);
        coset_shifted_weights(st.coset_indices, st.r_powers, N, st.n / l, shifted.data(), host_parallel_for);
        KZG_HIP_TRY(ctx, ctx->ml[4].reserve(N * 40));
        r->d_w2 = ctx->ml[4].as<uint4>();
        r->d_ci = reinterpret_cast<uint64_t*>(ctx->ml[4].as<uint8_t>() + N * 32);
        KZG_HIP_TRY(ctx, hipMemcpyAsync(r->d_w2, shifted.data(), N * 32, hipMemcpyHostToDevice, ctx->stream));
        KZG_HIP_TRY(ctx, hipMemcpyAsync(r->d_ci, st.commitment_indices, N * 8, hipMemcpyHostToDevice, ctx->stream));
        rc = coset_item_rows_device(ctx, st.d_ys, st.d_k, st.d_w, N, st.n, l, r->transformed);
        if (rc != KZG_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
        KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                             // (`shifted` is in use until here)
        r->rows_ready = true;
    }
    out->lhs.clear();
    out->rhs.clear();
    if (S == 0) return KZG_OK;
    rc = locate_upload_plan(ctx, plan);
    if (rc == KZG_OK) rc = coset_seg_sums_device(ctx, st.d_ys, plan, l);
    if (rc != KZG_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }            // (the plan's arrays are in flight)
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                                 // the MSM launches run on the slots' streams
    std::vector<uint64_t> interp_xy(8 * S);
    rc = commit_batch_device(ctx, srs, ctx->ml[0].p, l, S, interp_xy.data(), nullptr);
    if (rc != KZG_OK) return rc;
    std::vector<uint64_t> sums(32 * S);
    rc = locate_point_sums_device(ctx, st.d_bases + 4 * N, r->d_ci, st.d_w, r->d_w2, plan, sums.data(), N);
    if (rc != KZG_OK) return rc;
    out->lhs.resize(S);
    out->rhs.resize(S);
    const size_t per = 256;
    host_parallel_for((S + per - 1) / per, [&](size_t c) {
        for (size_t j = c * per; j < std::min(S, (c + 1) * per); ++j) {
            Xyzz b;
            memcpy(&out->lhs[j], sums.data() + 32 * j, 128);
            memcpy(&b, sums.data() + 32 * j + 16, 128);
            Xyzz i = xyzz_from_affine_wire(interp_xy.data() + 8 * j);
            i.y = neg(i.y);
            out->rhs[j] = xyzz_add(b, i);
        }
    });
    return KZG_OK;
}

// The search of host_locate.h over the segments' pairs: seg_ok[j] = 1 for a good segment, *bad = the bad ones.  Returns the pairing checks.
size_t group_search(const GroupSums& gs, const kzg_host::G2& g2_tau_l, uint8_t* seg_ok, size_t* bad) {
    using namespace kzg_host;
    struct Ops {
        Xyzz zero() const { return xyzz_inf(); }
        Xyzz add(const Xyzz& a, const Xyzz& b) const { return xyzz_add(a, b); }
        Xyzz sub(const Xyzz& a, Xyzz b) const { b.y = neg(b.y); return xyzz_add(a, b); }
    };
    const G2 g2 = g2_generator();
    auto holds = [&](const Xyzz& lhs, const Xyzz& rhs) {
        uint64_t a[8], b[8];
        xyzz_to_affine(lhs, a, nullptr);
        xyzz_to_affine(rhs, b, nullptr);
        return pairings_verify_pooled(g1_from_wire(a), g2_tau_l, g1_from_wire(b), g2);
    };
    return locate_search(gs.lhs.data(), gs.rhs.data(), gs.lhs.size(), Ops(), holds, seg_ok, bad);
}

// count points -> affine wire words and identity flags, one inversion per 256 points, chunks on the host pool
void xyzz_to_affine_many(const kzg_host::Xyzz* p, size_t count, uint64_t* out_xy, uint8_t* out_inf) {
    const size_t per = 256;
    host_parallel_for((count + per - 1) / per, [&](size_t c) {
        const size_t a = c * per, b = std::min(count, (c + 1) * per);
        kzg_host::xyzz_batch_to_affine(p + a, b - a, out_xy + 8 * a);
        for (size_t j = a; j < b; ++j) out_inf[j] = kzg_host::is_inf(p[j]) ? 1 : 0;
    });
}

// The located pass over the segments' pairs by the context's mode (kzg_ctx_set_locate_pairings).  Mode 0: group_search, as it always was.
// Mode 1: the root [0, S) on the host, so that a batch whose root holds costs one check and no device work; after a failing root over more
// than one segment EVERY segment's own equation e(L_j, [tau^l]_2) e(-R_j, G2) = 1 goes to the device as one batch (pairing.hip; the sums to
// affine with one inversion per 256), and the verdicts are seg_ok: 1 + S checks.  A failing root over ONE segment names it without another check.
// locked: the caller holds ctx->mu (the batch works in the context's buffers, so it is taken here otherwise).
int32_t group_locate(kzg_ctx* ctx, bool locked, const GroupSums& gs, const kzg_host::G2& g2_tau_l, uint8_t* seg_ok, size_t* bad, size_t* checks) {
    using namespace kzg_host;
    if (ctx->locate_pairings.load() == 0) { *checks = group_search(gs, g2_tau_l, seg_ok, bad); return KZG_OK; }
    const size_t S = gs.lhs.size();
    *bad = 0; *checks = 0;
    if (S == 0) return KZG_OK;
    std::vector<Xyzz> sums(2 * S);                                                       // L_0 .. L_(S-1), then -R_0 .. -R_(S-1)
    Xyzz tl = xyzz_inf(), tr = xyzz_inf();
    for (size_t j = 0; j < S; ++j) {
        sums[j] = gs.lhs[j];
        sums[S + j] = gs.rhs[j];
        sums[S + j].y = neg(sums[S + j].y);
        tl = xyzz_add(tl, gs.lhs[j]); tr = xyzz_add(tr, gs.rhs[j]);
    }
    {
        uint64_t a[8], b[8];
        xyzz_to_affine(tl, a, nullptr);
        xyzz_to_affine(tr, b, nullptr);
        *checks = 1;
        if (pairings_verify_pooled(g1_from_wire(a), g2_tau_l, g1_from_wire(b), g2_generator())) { memset(seg_ok, 1, S); return KZG_OK; }
    }
    if (S == 1) { seg_ok[0] = 0; *bad = 1; return KZG_OK; }
    std::vector<uint64_t> xy(16 * S);
    std::vector<uint8_t> inf(2 * S);
    xyzz_to_affine_many(sums.data(), 2 * S, xy.data(), inf.data());
    uint64_t q_tau[16], q_gen[16];
    g2_to_wire(g2_tau_l, q_tau);
    g2_to_wire(g2_generator(), q_gen);
    std::unique_lock<std::mutex> lk(ctx->mu, std::defer_lock);
    if (!locked) { lk.lock(); KZG_HIP_TRY(ctx, hipSetDevice(ctx->device)); }
    const size_t slice = PAIRING_RUN_MAX_PAIRS / 2;                                    // two pairs per check
    std::vector<uint64_t> g1s, g2s, offs;
    for (size_t lo = 0; lo < S; lo += slice) {
        const size_t m = std::min(slice, S - lo);
        g1s.assign(16 * m, 0); g2s.resize(32 * m); offs.resize(m + 1);
        for (size_t j = 0; j < m; ++j) {
            if (!inf[lo + j]) memcpy(&g1s[16 * j], &xy[8 * (lo + j)], 64);
            if (!inf[S + lo + j]) memcpy(&g1s[16 * j + 8], &xy[8 * (S + lo + j)], 64);
            memcpy(&g2s[32 * j], q_tau, 128); memcpy(&g2s[32 * j + 16], q_gen, 128);
            offs[j] = 2 * j;
        }
        offs[m] = 2 * m;
        const int32_t rc = pairing_batch_run(ctx, g1s.data(), g2s.data(), offs.data(), m, 2 * m, seg_ok + lo, nullptr, nullptr);
        if (rc != KZG_OK) return rc;
    }
    for (size_t j = 0; j < S; ++j) *bad += seg_ok[j] ? 0 : 1;
    *checks += S;
    return KZG_OK;
}

// ---- batches of mixed shapes (host_coset_mixed.h, multiverify.hip coset_interpolate_rlc_mixed_device) ----------------------------------------
// The plan of one call and where its items lie on the device.  Values, coset indices and weights go up ONCE in the caller's order; the kernels
// reach an item through the plan's permutation.  ctx->mv[0]: the ragged values; ctx->mv[1]: N weights | N coset indices | the plan's tables
// (`aux`: perm | val_off | workgroup classes of the two launches | MixedClassDev per class | MixedRow per row); ctx->mv[2]: l_max coefficients.
struct MixedStage {
    kzg_host::MixedPlan plan;
    std::vector<uint32_t> aux;                   // (in use until the stream is drained)
    uint4* d_ys = nullptr; uint4* d_w = nullptr; uint64_t* d_k = nullptr;
    MixedDevTables t{};
};

// enqueued on ctx->stream; the caller holds ctx->mu and has set the device
int32_t mixed_upload(kzg_ctx* ctx, const uint64_t* ys, const uint64_t* coset_indices, const uint64_t* weights, MixedStage* m) {
    const kzg_host::MixedPlan& p = m->plan;
    const size_t N = p.count;
    std::vector<uint32_t>& aux = m->aux;
    aux.clear();
    const size_t at_perm = 0, at_off = N, at_wg0 = 2 * N, at_wg1 = at_wg0 + p.wg_class[0].size(), at_cls = at_wg1 + p.wg_class[1].size(),
                 at_rows = at_cls + 8 * p.cls.size(), words = at_rows + 2 * p.rows.size();
    static_assert(sizeof(kzg_host::MixedClassDev) == 32 && sizeof(kzg_host::MixedRow) == 8, "the tables go up as u32 words");
    aux.resize(words);
    if (N) { memcpy(&aux[at_perm], p.perm.data(), N * 4); memcpy(&aux[at_off], p.val_off.data(), N * 4); }
    if (!p.wg_class[0].empty()) memcpy(&aux[at_wg0], p.wg_class[0].data(), p.wg_class[0].size() * 4);
    if (!p.wg_class[1].empty()) memcpy(&aux[at_wg1], p.wg_class[1].data(), p.wg_class[1].size() * 4);
    if (!p.cls.empty()) memcpy(&aux[at_cls], p.cls.data(), p.cls.size() * 32);
    if (!p.rows.empty()) memcpy(&aux[at_rows], p.rows.data(), p.rows.size() * 8);
    KZG_HIP_TRY(ctx, ctx->mv[0].reserve(std::max<size_t>(p.total_values * 32, 32)));
    KZG_HIP_TRY(ctx, ctx->mv[1].reserve(N * 40 + words * 4 + 64));
    KZG_HIP_TRY(ctx, ctx->mv[2].reserve(std::max<size_t>(p.l_max * 32, 32)));
    m->d_ys = ctx->mv[0].as<uint4>();
    m->d_w = ctx->mv[1].as<uint4>();
    m->d_k = reinterpret_cast<uint64_t*>(ctx->mv[1].as<uint8_t>() + N * 32);
    const uint32_t* d_aux = reinterpret_cast<const uint32_t*>(ctx->mv[1].as<uint8_t>() + N * 40);
    m->t.perm = d_aux + at_perm; m->t.val_off = d_aux + at_off; m->t.wg_class[0] = d_aux + at_wg0; m->t.wg_class[1] = d_aux + at_wg1;
    m->t.classes = d_aux + at_cls; m->t.rows = d_aux + at_rows;
    if (N) {
        KZG_HIP_TRY(ctx, hipMemcpyAsync(m->d_ys, ys, p.total_values * 32, hipMemcpyHostToDevice, ctx->stream));
        KZG_HIP_TRY(ctx, hipMemcpyAsync(m->d_w, weights, N * 32, hipMemcpyHostToDevice, ctx->stream));
        KZG_HIP_TRY(ctx, hipMemcpyAsync(m->d_k, coset_indices, N * 8, hipMemcpyHostToDevice, ctx->stream));
        KZG_HIP_TRY(ctx, hipMemcpyAsync(const_cast<uint32_t*>(d_aux), aux.data(), words * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    return KZG_OK;
}

}  // namespace

extern "C" {

int32_t kzg_compute_multiproof_r_powers(const uint64_t* commitments_xy_mont, size_t n_commitments, const uint64_t* commitment_indices,
                                        const uint64_t* coset_indices, const uint64_t* ys_mont, const uint64_t* proofs_xy_mont,
                                        size_t count, size_t n, size_t chunk_len, uint64_t* out_r_powers_mont) {
    if (count == 0) return KZG_OK;
    if (!commitment_indices || !coset_indices || !ys_mont || !proofs_xy_mont || !out_r_powers_mont || (n_commitments && !commitments_xy_mont)) return KZG_ERR_INVALID_ARG;
    if (chunk_len == 0 || count > ((size_t)1 << 28) / chunk_len) return chunk_len == 0 ? KZG_ERR_INVALID_ARG : KZG_ERR_TOO_LARGE;
    multiproof_r_powers_host(commitments_xy_mont, n_commitments, commitment_indices, coset_indices, ys_mont, proofs_xy_mont, count, n, chunk_len, out_r_powers_mont, host_parallel_for);
    return KZG_OK;
}

int32_t kzg_compute_multiproof_r_powers_device(kzg_ctx* ctx, const uint64_t* commitments_xy_mont, size_t n_commitments, const uint64_t* commitment_indices,
                                               const uint64_t* coset_indices, const uint64_t* ys_mont, const uint64_t* proofs_xy_mont,
                                               size_t count, size_t n, size_t chunk_len, uint64_t* out_r_powers_mont) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    if (count == 0) return KZG_OK;
    if (!commitment_indices || !coset_indices || !ys_mont || !proofs_xy_mont || !out_r_powers_mont || (n_commitments && !commitments_xy_mont)) return KZG_ERR_INVALID_ARG;
    if (chunk_len == 0 || count > ((size_t)1 << 28) / chunk_len) return chunk_len == 0 ? KZG_ERR_INVALID_ARG : KZG_ERR_TOO_LARGE;
    CosetStage st;                                                                       // mode 2: the device, whatever the context's setting
    const int32_t rc = coset_stage_words(ctx, commitments_xy_mont, n_commitments, commitment_indices, coset_indices, ys_mont, proofs_xy_mont, count, n, chunk_len, nullptr, false, &st, 2);
    if (rc == KZG_OK) memcpy(out_r_powers_mont, st.r_powers, count * 32);
    return rc;
}

int32_t kzg_coset_interpolate_rlc(kzg_ctx* ctx, const uint64_t* ys_mont, const uint64_t* coset_indices, const uint64_t* weights_mont,
                                  size_t count, size_t n, size_t chunk_len, uint64_t* out_coeffs_mont) {
    if (!ctx || !out_coeffs_mont) return KZG_ERR_INVALID_ARG;
    if (count && (!ys_mont || !coset_indices || !weights_mont)) return KZG_ERR_INVALID_ARG;
    int32_t rc = coset_domain_check(n, chunk_len);
    if (rc != KZG_OK) return rc;
    for (size_t i = 0; i < count; ++i) if (coset_indices[i] >= n / chunk_len) return KZG_ERR_INVALID_ARG;
    if (count > ((size_t)1 << 28) / chunk_len) return KZG_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t l = chunk_len;
    uint4* d_w = nullptr;
    uint64_t* d_k = nullptr;
    rc = coset_upload(ctx, ys_mont, coset_indices, weights_mont, count, l, &d_w, &d_k);
    if (rc == KZG_OK) rc = coset_interpolate_rlc_device(ctx, ctx->mv[0].as<uint4>(), d_k, d_w, count, n, l, ctx->mv[2].as<uint4>());
    if (rc != KZG_OK) return rc;
    KZG_HIP_TRY(ctx, hipMemcpyAsync(out_coeffs_mont, ctx->mv[2].p, l * 32, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KZG_OK;
}

// the batch equation on wire words (coset_batch_tail states it)
int32_t kzg_verify_multiproof_batch(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* commitments_xy_mont, size_t n_commitments,
                                    const uint64_t* commitment_indices, const uint64_t* coset_indices, const uint64_t* ys_mont,
                                    const uint64_t* proofs_xy_mont, size_t count, size_t n, size_t chunk_len,
                                    const uint64_t* r_powers_mont, const uint64_t* g2_tau_l_mont, int32_t* out_ok) {
    int32_t rc = multiproof_batch_checks(ctx, srs, !out_ok, !commitments_xy_mont || !commitment_indices || !coset_indices || !ys_mont || !proofs_xy_mont,
                                         !g2_tau_l_mont && chunk_len != 1, n_commitments, commitment_indices, coset_indices, count, n, chunk_len, nullptr, 0, false);
    if (rc != KZG_OK) return rc;
    if (count == 0) { *out_ok = 1; return KZG_OK; }
    const auto t0 = Clock::now();
    kzg_host::G2 g2_tau_l;
    const bool g2_ok = load_g2_tau(g2_tau_l_mont, &g2_tau_l);                            // reported after an off-curve G1 point, as verify_batch_core does
    CosetStage st;
    rc = coset_stage_words(ctx, commitments_xy_mont, n_commitments, commitment_indices, coset_indices, ys_mont, proofs_xy_mont, count, n, chunk_len, r_powers_mont, true, &st);
    if (rc != KZG_OK) return rc;
    if (!g2_ok) return KZG_ERR_G2_TAU_NOT_ON_CURVE;
    CosetTailTimes t;
    rc = coset_batch_tail(ctx, srs, st, g2_tau_l, out_ok, &t);
    if (rc != KZG_OK) return rc;
    if (opts().vb_trace)
        fprintf(stderr, "kzg_verify_multiproof_batch N=%zu l=%zu M=%zu: r_powers%s %.3f ms, upload %.3f ms, interpolation kernel %.3f ms, coefficient MSM %.3f ms, "
                "host scalars + proof / commitment MSMs %.3f ms, point sums + pairing %.3f ms, call %.3f ms\n", count, chunk_len, n_commitments, st.rp_path, st.ms[0], st.ms[1],
                ms_between(t.start, t.interpolated), ms_between(t.interpolated, t.coeff_msm), ms_between(t.coeff_msm, t.point_msms), ms_between(t.point_msms, Clock::now()),
                ms_between(t0, Clock::now()));
    return KZG_OK;
}

// ---- batches of mixed shapes ------------------------------------------------------------------------------------------------------------
int32_t kzg_compute_multiproof_r_powers_mixed(const uint64_t* commitments_xy_mont, size_t n_commitments, const uint64_t* commitment_indices, const uint64_t* class_n,
                                              const uint64_t* class_chunk_len, size_t n_classes, const uint64_t* class_indices, const uint64_t* coset_indices,
                                              const uint64_t* ys_mont, const uint64_t* proofs_xy_mont, size_t count, uint64_t* out_r_powers_mont) {
    if (count == 0) return KZG_OK;
    if (!commitment_indices || !class_n || !class_chunk_len || !class_indices || !coset_indices || !ys_mont || !proofs_xy_mont || !out_r_powers_mont ||
        (n_commitments && !commitments_xy_mont))
        return KZG_ERR_INVALID_ARG;
    size_t total = 0;
    for (size_t i = 0; i < count; ++i) {
        if (class_indices[i] >= n_classes || class_chunk_len[class_indices[i]] == 0) return KZG_ERR_INVALID_ARG;
        if (class_chunk_len[class_indices[i]] > kzg_host::MIXED_MAX_VALUES) return KZG_ERR_TOO_LARGE;
        total += (size_t)class_chunk_len[class_indices[i]];
        if (total > kzg_host::MIXED_MAX_VALUES) return KZG_ERR_TOO_LARGE;
    }
    std::vector<uint32_t> off;
    kzg_host::mixed_value_offsets(class_chunk_len, class_indices, count, &off);
    kzg_host::multiproof_r_powers_mixed_host(commitments_xy_mont, n_commitments, commitment_indices, class_n, class_chunk_len, n_classes, class_indices, coset_indices,
                                             ys_mont, off.data(), proofs_xy_mont, count, out_r_powers_mont, host_parallel_for);
    return KZG_OK;
}

int32_t kzg_coset_interpolate_rlc_mixed(kzg_ctx* ctx, const uint64_t* class_n, const uint64_t* class_chunk_len, size_t n_classes, const uint64_t* class_indices,
                                        const uint64_t* coset_indices, const uint64_t* ys_mont, const uint64_t* weights_mont, size_t count, uint64_t* out_coeffs_mont) {
    const bool bad = !ctx || !out_coeffs_mont || (n_classes && (!class_n || !class_chunk_len)) || (count && (!class_indices || !coset_indices || !ys_mont || !weights_mont));
    size_t l_max = 0, total = 0;
    int32_t rc = kzg_host::mixed_checks(bad, class_n, class_chunk_len, n_classes, SIZE_MAX, 0, nullptr, class_indices, coset_indices, count, nullptr, &l_max, &total);
    if (rc != KZG_OK) return rc;
    if (l_max == 0) return KZG_OK;                                                       // (no class: no coefficient)
    MixedStage m;
    kzg_host::mixed_plan(class_n, class_chunk_len, n_classes, class_indices, count, &m.plan);
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = mixed_upload(ctx, ys_mont, coset_indices, weights_mont, &m);
    if (rc == KZG_OK) rc = coset_interpolate_rlc_mixed_device(ctx, m.plan, m.d_ys, m.d_k, m.d_w, m.t, ctx->mv[2].as<uint4>());
    if (rc != KZG_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }            // (the plan's tables are in flight)
    KZG_HIP_TRY(ctx, hipMemcpyAsync(out_coeffs_mont, ctx->mv[2].p, l_max * 32, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KZG_OK;
}

// The batch equation for items of mixed shapes: class s is (n_s, l_s), item i has the class s_i.  With the weights r_i,
//     A_t = sum_{i : l_{s_i} > t} r_i w_{s_i}^(-k_i t) IFFT_{l_{s_i}}(ys_i)_t   (t < l_max),      L_d = sum_{i : l_{s_i} = d} r_i pi_i   per DISTINCT chunk length d,
//     R = sum_i r_i C_{c_i} - sum_t A_t [tau^t]_1 + sum_i r_i w_{s_i}^(k_i l_{s_i}) pi_i,         accept <=> prod_d e(L_d, [tau^d]_2) e(-R, G2) = 1:
// 1 + (distinct chunk lengths that have items) pairs whatever the item count; only the G2 side depends on the chunk length.  The bases hold the
// proofs sorted by chunk length (the plan's permutation, which is sorted by class and by length at once): each L_d is a contiguous variable-base
// MSM, and the second copy of the proofs with the commitments behind it is ONE MSM for the two point sums of R.
int32_t kzg_verify_multiproof_batch_mixed(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* commitments_xy_mont, size_t n_commitments, const uint64_t* commitment_indices,
                                          const uint64_t* class_n, const uint64_t* class_chunk_len, size_t n_classes, const uint64_t* class_indices,
                                          const uint64_t* coset_indices, const uint64_t* ys_mont, const uint64_t* proofs_xy_mont, size_t count,
                                          const uint64_t* r_powers_mont, const uint64_t* g2_tau_l_mont, int32_t* out_ok) {
    using namespace kzg_host;
    const bool bad = !ctx || !srs || !out_ok || (n_classes && (!class_n || !class_chunk_len || !g2_tau_l_mont)) ||
                     (count && (!commitments_xy_mont || !commitment_indices || !class_indices || !coset_indices || !ys_mont || !proofs_xy_mont)) ||
                     srs->ctx != ctx || srs->lagrange_of != 0;
    size_t l_max = 0, total = 0;
    int32_t rc = mixed_checks(bad, class_n, class_chunk_len, n_classes, bad ? 0 : srs->n, n_commitments, commitment_indices, class_indices, coset_indices, count,
                              g2_tau_l_mont, &l_max, &total);
    if (rc != KZG_OK) return rc;
    if (count == 0) { *out_ok = 1; return KZG_OK; }
    const bool trace = opts().vb_trace != 0;
    const auto t0 = Clock::now();
    const size_t N = count, M = n_commitments;
    MixedStage m;
    mixed_plan(class_n, class_chunk_len, n_classes, class_indices, N, &m.plan);
    const MixedPlan& p = m.plan;
    // the G2 point of every chunk length that has items, taken from the first class of that length (the others carry the same bits); a point off the
    // twist is reported behind an off-curve G1 point, for the first class in class order that has items
    std::vector<G2> g2s(p.lens.size() + 1);
    for (size_t d = 0; d < p.lens.size(); ++d) g2s[d] = g2_from_wire(g2_tau_l_mont + 16 * p.lens[d].g2_class);
    g2s[p.lens.size()] = g2_generator();
    bool g2_ok = true;
    for (size_t s = 0; s < n_classes && g2_ok; ++s)
        if (p.cls[s].count) g2_ok = g2_on_curve(g2_from_wire(g2_tau_l_mont + 16 * s));
    // the weights: supplied, or derived on the host pool BEFORE ctx->mu is taken (threads that share a context overlap there)
    const auto t_plan = Clock::now();
    std::vector<uint64_t> derived;
    if (!r_powers_mont) {
        RoctxRange range("kzg:multiproof_verify_mixed:r_powers (host)");
        derived.resize(4 * N);
        multiproof_r_powers_mixed_host(commitments_xy_mont, M, commitment_indices, class_n, class_chunk_len, n_classes, class_indices, coset_indices, ys_mont,
                                       p.val_off.data(), proofs_xy_mont, N, derived.data(), host_parallel_for);
        r_powers_mont = derived.data();
    }
    const auto t_rp = Clock::now();
    std::unique_lock<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_refused(ctx, true)) return KZG_ERR_INVALID_ARG;
    rc = mixed_upload(ctx, ys_mont, coset_indices, r_powers_mont, &m);
    if (rc != KZG_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    // the points, validated on their way into the device format: proofs by chunk length | the same again | commitments (synchronised)
    KZG_HIP_TRY(ctx, ctx->msm.bases.reserve((2 * N + M) * 64));
    uint4* d_bases = ctx->msm.bases.as<uint4>();
    {
        std::vector<uint64_t> twice(2 * N * 8);
        for (size_t j = 0; j < N; ++j) {
            memcpy(twice.data() + 8 * j, proofs_xy_mont + 8 * (size_t)p.perm[j], 64);
            memcpy(twice.data() + 8 * (N + j), proofs_xy_mont + 8 * (size_t)p.perm[j], 64);
        }
        rc = coset_upload_points(ctx, twice.data(), 2 * N, commitments_xy_mont, M, d_bases, d_bases + 4 * 2 * N);
        if (rc != KZG_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    }
    if (!g2_ok) return KZG_ERR_G2_TAU_NOT_ON_CURVE;
    const auto t_up = Clock::now();
    // 1. the l_max coefficients A_t (left on the device), 2. their MSM over srs[0 .. l_max)
    rc = coset_interpolate_rlc_mixed_device(ctx, p, m.d_ys, m.d_k, m.d_w, m.t, ctx->mv[2].as<uint4>());
    if (rc != KZG_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    if (trace) KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const auto t_interp = Clock::now();
    uint64_t interp_xy[8];
    uint8_t interp_inf = 0;
    rc = msm_srs_locked(ctx, srs, 0, ctx->mv[2].p, true, l_max, interp_xy, &interp_inf, nullptr);
    if (rc != KZG_OK) return rc;
    const auto t_msm = Clock::now();
    // 3. host scalars in the order of the bases, 4. one MSM per distinct chunk length over the first copy, one over the second copy and the commitments
    std::vector<uint64_t> class_m(n_classes), scalars((2 * N + M) * 4);
    for (size_t s = 0; s < n_classes; ++s) class_m[s] = class_n[s] / class_chunk_len[s];
    coset_batch_scalars_mixed(class_m.data(), n_classes, class_indices, coset_indices, commitment_indices, r_powers_mont, p.perm.data(), N, M, scalars.data(),
                              host_parallel_for);
    KZG_HIP_TRY(ctx, ctx->msm.scalars.reserve((2 * N + M) * 32 + 32));
    const uint4* d_scalars = ctx->msm.scalars.as<uint4>();
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->msm.scalars.p, scalars.data(), (2 * N + M) * 32, hipMemcpyHostToDevice, ctx->stream));
    std::vector<G1> g1s(p.lens.size() + 1);
    uint64_t sum_xy[8];
    uint8_t inf = 0;
    for (size_t d = 0; d < p.lens.size() && rc == KZG_OK; ++d) {
        rc = msm_run_batch(ctx, d_bases + 4 * p.lens[d].first, d_scalars + 2 * p.lens[d].first, p.lens[d].count, 1, sum_xy, &inf);
        if (rc == KZG_OK) g1s[d] = g1_from_wire(sum_xy);
    }
    if (rc == KZG_OK) rc = msm_run_batch(ctx, d_bases + 4 * N, d_scalars + 2 * N, N + M, 1, sum_xy, &inf);
    if (rc != KZG_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }            // (`scalars` is in use until the stream is drained)
    lk.unlock();
    const auto t_pts = Clock::now();
    // 5. ONE pooled product of 1 + (distinct chunk lengths) pairings
    g1s[p.lens.size()] = g1_neg(g1_add(g1_from_wire(sum_xy), g1_neg(g1_from_wire(interp_xy))));
    *out_ok = pairings_product_is_one(g1s.data(), g2s.data(), (int)g1s.size(), host_parallel_for) ? 1 : 0;
    if (trace)
        fprintf(stderr, "kzg_verify_multiproof_batch_mixed N=%zu classes=%zu lengths=%zu l_max=%zu M=%zu: r_powers%s %.3f ms, plan + upload %.3f ms, interpolation kernels %.3f ms, "
                "coefficient MSM %.3f ms, host scalars + proof / commitment MSMs %.3f ms, point sums + pairings %.3f ms, call %.3f ms\n", N, n_classes, p.lens.size(), l_max, M,
                derived.empty() ? " (supplied)" : " (host)", ms_between(t_plan, t_rp), ms_between(t0, t_plan) + ms_between(t_rp, t_up), ms_between(t_up, t_interp), ms_between(t_interp, t_msm),
                ms_between(t_msm, t_pts), ms_between(t_pts, Clock::now()), ms_between(t0, Clock::now()));
    return KZG_OK;
}

int32_t kzg_verify_multiproof(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t commitment_xy_mont[8], const uint64_t proof_xy_mont[8],
                              uint64_t coset_index, const uint64_t* ys_mont, size_t n, size_t chunk_len,
                              const uint64_t* g2_tau_l_mont, int32_t* out_ok) {
    if (!commitment_xy_mont || !proof_xy_mont || !ys_mont) return KZG_ERR_INVALID_ARG;
    const uint64_t zero = 0;
    uint64_t one_w[4];
    kzg_host::fr_one(one_w);
    return kzg_verify_multiproof_batch(ctx, srs, commitment_xy_mont, 1, &zero, &coset_index, ys_mont, proof_xy_mont, 1, n, chunk_len, one_w, g2_tau_l_mont, out_ok);
}

// kzg_verify_multiproof_batch on items in their serialized form: the same equation, weights and verdict, with the decode inside the call
int32_t kzg_verify_multiproof_batch_bytes(kzg_ctx* ctx, const kzg_srs* srs, const uint8_t* commitments_be, size_t n_commitments, const uint64_t* commitment_indices,
                                          const uint64_t* coset_indices, const uint8_t* ys_be, const uint8_t* proofs_be, size_t count, size_t n, size_t chunk_len,
                                          const uint64_t* r_powers_mont, const uint64_t* g2_tau_l_mont, int32_t* out_ok, uint64_t* out_r_powers_mont,
                                          uint64_t* bad_index, int32_t* bad_array) {
    int32_t rc = multiproof_batch_checks(ctx, srs, !out_ok, !commitments_be || !commitment_indices || !coset_indices || !ys_be || !proofs_be,
                                         !g2_tau_l_mont && chunk_len != 1, n_commitments, commitment_indices, coset_indices, count, n, chunk_len, nullptr, 0, false);
    if (rc != KZG_OK) return rc;
    if (count == 0) { *out_ok = 1; return KZG_OK; }
    const auto t0 = Clock::now();
    kzg_host::G2 g2_tau_l;
    const bool g2_ok = load_g2_tau(g2_tau_l_mont, &g2_tau_l);                            // reported after the bytes, as the decoded entry reports it after the points
    CosetStage st;
    rc = coset_stage_bytes(ctx, "kzg_verify_multiproof_batch_bytes", commitments_be, n_commitments, commitment_indices, coset_indices, ys_be, proofs_be, count, n, chunk_len,
                           r_powers_mont, g2_ok, bad_index, bad_array, &st);
    if (rc != KZG_OK) return rc;
    CosetTailTimes t;
    rc = coset_batch_tail(ctx, srs, st, g2_tau_l, out_ok, &t);
    if (rc != KZG_OK) return rc;
    if (out_r_powers_mont) memcpy(out_r_powers_mont, st.r_powers, count * 32);
    if (opts().vb_trace)
        fprintf(stderr, "kzg_verify_multiproof_batch_bytes N=%zu l=%zu M=%zu: decode (staging, uploads, decode kernels; host r_powers beside them %.3f ms) %.3f ms, "
                "r_powers%s %.3f ms, interpolation kernel %.3f ms, coefficient MSM %.3f ms, host scalars + proof / commitment MSMs %.3f ms, "
                "point sums + pairing %.3f ms, call %.3f ms\n", count, chunk_len, n_commitments, st.ms[0], st.ms[1], st.rp_path, st.ms[2], ms_between(t.start, t.interpolated),
                ms_between(t.interpolated, t.coeff_msm), ms_between(t.coeff_msm, t.point_msms), ms_between(t.point_msms, Clock::now()), ms_between(t0, Clock::now()));
    return KZG_OK;
}

// The retriever's call: kzg_verify_multiproof_batch_bytes on the chunks of `blobs` blobs (item b count + j: commitment b, coset j of the blob's index
// row) and, if the batch is accepted, kzg_recover_from_cosets_batch_bytes on the same values -- uploaded ONCE.  Where the recovery reads them: the
// front end leaves the value bytes in ctx->cb[0] and the decoded words in ctx->mv[0].  The interpolation reads mv[0] in place for l <= 1024 but
// transforms it in place above that (multiverify.hip: ntt_run per coset), while nothing behind the front end writes cb[0] (the device transcript and
// the MSMs read it or work elsewhere): the bytes are what every shape leaves intact, so the scatter kernel decodes them on load, one path for all l
// at one field product per value in a kernel bound by its loads.  The verifier has already refused every value >= r, so the recovery meets none.
// Checks: the recovery's table on the host, then the verifier's table on the host, nothing launched before both; then the verifier's device-side
// refusals in its order.  *out_ok = 0: KZG_OK, no recovery kernel runs, out_polys_be / out_consistent are not written.  Device memory: what both
// halves use, side by side (the verifier's cb / mv / msm workspaces stay reserved while the recovery's rc / rc_ntt ones are filled).
int32_t kzg_retrieve_blobs_bytes(kzg_ctx* ctx, const kzg_srs* srs, const uint8_t* commitments_be, const uint64_t* coset_indices, size_t index_rows, const uint8_t* ys_be,
                                 const uint8_t* proofs_be, size_t blobs, size_t count, size_t n, size_t chunk_len, size_t degree_bound, int32_t eval_form, size_t out_len,
                                 const uint64_t* r_powers_mont, const uint64_t* g2_tau_l_mont, int32_t* out_ok, uint8_t* out_polys_be, int32_t* out_consistent,
                                 uint64_t* bad_index, int32_t* bad_array) {
    int32_t rc = recover_bytes_check(!ctx || !ys_be || !coset_indices || !out_polys_be, coset_indices, index_rows, blobs, count, n, chunk_len, degree_bound,
                                     eval_form != 0, out_len);
    if (rc != KZG_OK) return rc;
    const size_t N = blobs * count;
    std::vector<uint64_t> cosets, rows;
    retrieve_items(coset_indices, index_rows, blobs, count, &cosets, &rows);
    rc = multiproof_batch_checks(ctx, srs, !out_ok, !commitments_be || !proofs_be, !g2_tau_l_mont && chunk_len != 1, blobs, rows.data(), cosets.data(), N, n, chunk_len,
                                 nullptr, 0, false);
    if (rc != KZG_OK) return rc;
    const auto t0 = Clock::now();
    kzg_host::G2 g2_tau_l;
    const bool g2_ok = load_g2_tau(g2_tau_l_mont, &g2_tau_l);
    CosetStage st;
    rc = coset_stage_bytes(ctx, "kzg_retrieve_blobs_bytes", commitments_be, blobs, rows.data(), cosets.data(), ys_be, proofs_be, N, n, chunk_len, r_powers_mont, g2_ok,
                           bad_index, bad_array, &st);
    if (rc != KZG_OK) return rc;
    CosetTailTimes t;
    rc = coset_batch_tail(ctx, srs, st, g2_tau_l, out_ok, &t);
    if (rc != KZG_OK) return rc;
    const auto t_verified = Clock::now();
    if (*out_ok) {
        RecoverBatchPlan plan;
        recover_batch_plan(coset_indices, index_rows, blobs, count, n, chunk_len, degree_bound, eval_form != 0, out_len, ctx->recover_group_bytes, &plan);
        uint32_t bad_word = 0xFFFFFFFFu;
        RecoverIo io;
        io.d_ys = ctx->cb[0].as<uint4>(); io.ys_be = true; io.out = out_polys_be; io.out_be = true; io.consistent = out_consistent; io.bad_word = &bad_word;
        rc = recover_run_batch(ctx, plan, io);
        if (rc == KZG_ERR_DESERIALIZE) {                                                 // (unreachable behind the verifier's decode; reported as that would)
            if (bad_array) *bad_array = 2;
            return coset_bytes_status(ctx, "kzg_retrieve_blobs_bytes", "value of item", bad_word, chunk_len, bad_index);
        }
        if (rc != KZG_OK) return rc;
    }
    if (opts().vb_trace)
        fprintf(stderr, "kzg_retrieve_blobs_bytes blobs=%zu count=%zu l=%zu: decode %.3f ms, r_powers%s %.3f ms, interpolation kernel %.3f ms, coefficient MSM %.3f ms, "
                "host scalars + proof / commitment MSMs %.3f ms, point sums + pairing %.3f ms, recover%s %.3f ms, call %.3f ms\n", blobs, count, chunk_len, st.ms[1],
                st.rp_path, st.ms[2], ms_between(t.start, t.interpolated), ms_between(t.interpolated, t.coeff_msm), ms_between(t.coeff_msm, t.point_msms),
                ms_between(t.point_msms, t_verified), *out_ok ? "" : " (skipped: the batch is refused)", ms_between(t_verified, Clock::now()), ms_between(t0, Clock::now()));
    return KZG_OK;
}

// For every group g of a partition of the items: L_g =sum_{i in g} r_i pi_i and R_g = sum_{i in g} (r_i C_{c_i} + r_i w^(k_i l) pi_i) -
// sum_t A_{g,t} [tau^t]_1; group g is good iff e(L_g, [tau^l]_2) = e(R_g, G2), and summed over the groups (L, R) is the (lhs, rhs) of
// kzg_verify_multiproof_batch above.
int32_t kzg_coset_group_sums(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* commitments_xy_mont, size_t n_commitments, const uint64_t* commitment_indices,
                             const uint64_t* coset_indices, const uint64_t* ys_mont, const uint64_t* proofs_xy_mont, size_t count, size_t n, size_t chunk_len,
                             const uint64_t* r_powers_mont, const uint64_t* group_indices, size_t n_groups, uint64_t* out_lhs_xy_mont,
                             uint8_t* out_lhs_is_infinity, uint64_t* out_rhs_xy_mont, uint8_t* out_rhs_is_infinity) {
    const bool out_null = n_groups && (!out_lhs_xy_mont || !out_lhs_is_infinity || !out_rhs_xy_mont || !out_rhs_is_infinity);
    int32_t rc = multiproof_batch_checks(ctx, srs, out_null, !commitments_xy_mont || !commitment_indices || !coset_indices || !ys_mont || !proofs_xy_mont || !group_indices,
                                         false, n_commitments, commitment_indices, coset_indices, count, n, chunk_len, group_indices, n_groups, true);
    if (rc != KZG_OK) return rc;
    GroupSums gs;
    if (count) {
        rc = coset_group_sums_core(ctx, srs, commitments_xy_mont, n_commitments, commitment_indices, coset_indices, ys_mont, proofs_xy_mont, count, n, chunk_len,
                                   r_powers_mont, group_indices, n_groups, &gs);
        if (rc != KZG_OK) return rc;
    }
    if (n_groups) {                                                                      // an empty group: the identity twice
        memset(out_lhs_xy_mont, 0, n_groups * 64);
        memset(out_rhs_xy_mont, 0, n_groups * 64);
        memset(out_lhs_is_infinity, 1, n_groups);
        memset(out_rhs_is_infinity, 1, n_groups);
    }
    const size_t S = gs.plan.segs.size();
    std::vector<uint64_t> xy(8 * S);
    std::vector<uint8_t> inf(S);
    for (int side = 0; side < 2; ++side) {
        xyzz_to_affine_many(side ? gs.rhs.data() : gs.lhs.data(), S, xy.data(), inf.data());
        uint64_t* out_xy = side ? out_rhs_xy_mont : out_lhs_xy_mont;
        uint8_t* out_inf = side ? out_rhs_is_infinity : out_lhs_is_infinity;
        for (size_t j = 0; j < S; ++j) {
            memcpy(out_xy + 8 * (size_t)gs.plan.segs[j], xy.data() + 8 * j, 64);
            out_inf[gs.plan.segs[j]] = inf[j];
        }
    }
    return KZG_OK;
}

int32_t kzg_verify_multiproof_batch_locate(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* commitments_xy_mont, size_t n_commitments,
                                           const uint64_t* commitment_indices, const uint64_t* coset_indices, const uint64_t* ys_mont,
                                           const uint64_t* proofs_xy_mont, size_t count, size_t n, size_t chunk_len, const uint64_t* r_powers_mont,
                                           const uint64_t* g2_tau_l_mont, const uint64_t* group_indices, size_t n_groups, uint8_t* out_group_ok,
                                           size_t* out_bad_groups, size_t* out_pairing_checks) {
    using namespace kzg_host;
    int32_t rc = multiproof_batch_checks(ctx, srs, !out_bad_groups || (n_groups && !out_group_ok),
                                         !commitments_xy_mont || !commitment_indices || !coset_indices || !ys_mont || !proofs_xy_mont || !group_indices,
                                         !g2_tau_l_mont && chunk_len != 1, n_commitments, commitment_indices, coset_indices, count, n, chunk_len, group_indices, n_groups, true);
    if (rc != KZG_OK) return rc;
    if (count == 0) {                                                                    // nothing to refuse: no device work, no pairing
        if (n_groups) memset(out_group_ok, 1, n_groups);
        *out_bad_groups = 0;
        if (out_pairing_checks) *out_pairing_checks = 0;
        return KZG_OK;
    }
    G2 g2_tau_l;
    const bool g2_ok = load_g2_tau(g2_tau_l_mont, &g2_tau_l);                            // reported after an off-curve G1 point, as the batch entry does
    GroupSums gs;
    rc = coset_group_sums_core(ctx, srs, commitments_xy_mont, n_commitments, commitment_indices, coset_indices, ys_mont, proofs_xy_mont, count, n, chunk_len,
                               r_powers_mont, group_indices, n_groups, &gs);
    if (rc != KZG_OK) return rc;
    if (!g2_ok) return KZG_ERR_G2_TAU_NOT_ON_CURVE;
    // the search runs over the non-empty groups: an empty group's pair is the identity twice, it holds and changes no range
    const auto t0 = Clock::now();
    const size_t S = gs.plan.segs.size();
    std::vector<uint8_t> seg_ok(S, 1);
    size_t bad = 0;
    size_t checks = 0;
    rc = group_locate(ctx, false, gs, g2_tau_l, seg_ok.data(), &bad, &checks);
    if (rc != KZG_OK) return rc;
    memset(out_group_ok, 1, n_groups);
    for (size_t j = 0; j < S; ++j) out_group_ok[gs.plan.segs[j]] = seg_ok[j];
    *out_bad_groups = bad;
    if (out_pairing_checks) *out_pairing_checks = checks;
    if (opts().vb_trace)
        fprintf(stderr, "kzg_verify_multiproof_batch_locate groups=%zu: search %.3f ms, %zu pairing checks, %zu bad groups\n", n_groups, ms_between(t0, Clock::now()), checks, bad);
    return KZG_OK;
}

// kzg_verify_multiproof_batch_locate on items in their serialized form: the bytes front end of kzg_verify_multiproof_batch_bytes, then the group
// sums over what it left on the device and the search of the decoded entry
int32_t kzg_verify_multiproof_batch_locate_bytes(kzg_ctx* ctx, kzg_srs* srs, const uint8_t* commitments_be, size_t n_commitments, const uint64_t* commitment_indices,
                                                 const uint64_t* coset_indices, const uint8_t* ys_be, const uint8_t* proofs_be, size_t count, size_t n, size_t chunk_len,
                                                 const uint64_t* r_powers_mont, const uint64_t* g2_tau_l_mont, const uint64_t* group_indices, size_t n_groups,
                                                 uint8_t* out_group_ok, size_t* out_bad_groups, size_t* out_pairing_checks, uint64_t* out_r_powers_mont,
                                                 uint64_t* bad_index, int32_t* bad_array) {
    int32_t rc = multiproof_batch_checks(ctx, srs, !out_bad_groups || (n_groups && !out_group_ok),
                                         !commitments_be || !commitment_indices || !coset_indices || !ys_be || !proofs_be || !group_indices,
                                         !g2_tau_l_mont && chunk_len != 1, n_commitments, commitment_indices, coset_indices, count, n, chunk_len, group_indices, n_groups, true);
    if (rc != KZG_OK) return rc;
    if (count == 0) {                                                                    // nothing to refuse: no device work, no pairing
        if (n_groups) memset(out_group_ok, 1, n_groups);
        *out_bad_groups = 0;
        if (out_pairing_checks) *out_pairing_checks = 0;
        return KZG_OK;
    }
    const auto t0 = Clock::now();
    kzg_host::G2 g2_tau_l;
    const bool g2_ok = load_g2_tau(g2_tau_l_mont, &g2_tau_l);                            // reported after the bytes, as the batch entry on bytes does
    GroupSums gs;
    rc = locate_plan(group_indices, count, n_groups, &gs.plan);
    if (rc != KZG_OK) return rc;
    CosetStage st;
    rc = coset_stage_bytes(ctx, "kzg_verify_multiproof_batch_locate_bytes", commitments_be, n_commitments, commitment_indices, coset_indices, ys_be, proofs_be, count, n,
                           chunk_len, r_powers_mont, g2_ok, bad_index, bad_array, &st);
    if (rc != KZG_OK) return rc;
    const auto t_staged = Clock::now();
    ResidentSums rs;
    rs.s = &st;
    rc = resident_group_sums(ctx, srs, &rs, gs.plan, &gs);
    if (rc != KZG_OK) return rc;
    st.lk.unlock();
    const auto t_sums = Clock::now();
    const size_t S = gs.plan.segs.size();
    std::vector<uint8_t> seg_ok(S, 1);
    size_t bad = 0;
    size_t checks = 0;
    rc = group_locate(ctx, false, gs, g2_tau_l, seg_ok.data(), &bad, &checks);
    if (rc != KZG_OK) return rc;
    if (n_groups) memset(out_group_ok, 1, n_groups);
    for (size_t j = 0; j < S; ++j) out_group_ok[gs.plan.segs[j]] = seg_ok[j];
    *out_bad_groups = bad;
    if (out_pairing_checks) *out_pairing_checks = checks;
    if (out_r_powers_mont) memcpy(out_r_powers_mont, st.r_powers, count * 32);
    if (opts().vb_trace)
        fprintf(stderr, "kzg_verify_multiproof_batch_locate_bytes N=%zu l=%zu M=%zu groups=%zu (non-empty %zu): decode + r_powers%s %.3f ms, group sums %.3f ms, "
                "search %.3f ms, %zu pairing checks, %zu bad groups\n", count, chunk_len, n_commitments, n_groups, S, st.rp_path, ms_between(t0, t_staged),
                ms_between(t_staged, t_sums), ms_between(t_sums, Clock::now()), checks, bad);
    return KZG_OK;
}

// The retriever's call that survives bad chunks: the front end of kzg_retrieve_blobs_bytes with per-item decode status, the batch equation once
// (refused items at weight 0), on a reject the located pass over the resident stage in two levels (blobs, then the single items of the bad
// blobs), and the recovery of every blob from its first use_count good items, reading the value bytes where the front end left them.
int32_t kzg_retrieve_blobs_bytes_tolerant(kzg_ctx* ctx, kzg_srs* srs, const uint8_t* commitments_be, const uint64_t* coset_indices, size_t index_rows,
                                          const uint8_t* ys_be, const uint8_t* proofs_be, size_t blobs, size_t count, size_t use_count, size_t n, size_t chunk_len,
                                          size_t degree_bound, int32_t eval_form, size_t out_len, const uint64_t* r_powers_mont, const uint64_t* g2_tau_l_mont,
                                          uint8_t* out_item_status, uint8_t* out_blob_status, size_t* out_bad_items, size_t* out_unrecovered,
                                          size_t* out_pairing_checks, uint8_t* out_polys_be, int32_t* out_consistent, uint64_t* out_r_powers_mont, uint64_t* bad_index,
                                          int32_t* bad_array) {
    int32_t rc = retrieve_tolerant_check(!ctx || !ys_be || !coset_indices || !out_polys_be || !out_item_status || !out_blob_status || !out_bad_items || !out_unrecovered,
                                         coset_indices, index_rows, blobs, count, use_count, n, chunk_len, degree_bound, eval_form != 0, out_len);
    if (rc != KZG_OK) return rc;
    const size_t N = blobs * count, l = chunk_len;
    std::vector<uint64_t> cosets, rows;
    retrieve_items(coset_indices, index_rows, blobs, count, &cosets, &rows);
    rc = multiproof_batch_checks(ctx, srs, false, !commitments_be || !proofs_be, !g2_tau_l_mont && chunk_len != 1, blobs, rows.data(), cosets.data(), N, n, chunk_len,
                                 nullptr, 0, false);
    if (rc != KZG_OK) return rc;
    const auto t0 = Clock::now();
    kzg_host::G2 g2_tau_l;
    const bool g2_ok = load_g2_tau(g2_tau_l_mont, &g2_tau_l);
    CosetStage st;
    std::vector<uint8_t> status;
    rc = coset_stage_bytes(ctx, "kzg_retrieve_blobs_bytes_tolerant", commitments_be, blobs, rows.data(), cosets.data(), ys_be, proofs_be, N, n, l, r_powers_mont, g2_ok,
                           bad_index, bad_array, &st, &status);
    if (rc != KZG_OK) return rc;
    CosetTailTimes t;
    int32_t ok = 0;
    rc = coset_batch_tail(ctx, srs, st, g2_tau_l, &ok, &t);
    if (rc != KZG_OK) return rc;
    const auto t_verified = Clock::now();
    size_t checks = 1;
    // ctx->mu (st.lk) stays held through the host-side searches below, so threads that share the context wait for their pairing checks too.  It
    // cannot be released in between: the located pass and the recovery read what the front end left in ctx->cb / mv / msm.bases, and any other
    // entry on this context would overwrite it.  A caller who wants overlap gives each thread its own context.
    if (!ok) {
        // level 1: groups = blobs (every item; a refused one adds the identity).  Level 2: groups = the single non-refused items of the bad blobs.
        // Two levels because the tree over all items costs 2 ceil(log2 N) checks per bad item AND sums, MSMs and point sums for N groups; the
        // blobs first cost ceil(log2 blobs) levels over `blobs` groups, and only the bad blobs' items become groups of their own.
        ResidentSums rs;
        rs.s = &st; rs.transformed = true;
        GroupSums gs;
        rc = locate_plan(rows.data(), N, blobs, &gs.plan);
        if (rc == KZG_OK) rc = resident_group_sums(ctx, srs, &rs, gs.plan, &gs);
        if (rc != KZG_OK) return rc;
        std::vector<uint8_t> blob_ok(blobs, 1);                                          // (count > 0: every blob is a segment, segment b = blob b)
        size_t bad_blobs = 0;
        size_t level_checks = 0;
        rc = group_locate(ctx, true, gs, g2_tau_l, blob_ok.data(), &bad_blobs, &level_checks);
        if (rc != KZG_OK) return rc;
        checks += level_checks;
        std::vector<uint32_t> items;
        for (size_t b = 0; b < blobs; ++b)
            if (!blob_ok[b])
                for (size_t j = 0; j < count; ++j) if (status[b * count + j] == RETRIEVE_ITEM_GOOD) items.push_back((uint32_t)(b * count + j));
        if (!items.empty()) {
            std::vector<uint64_t> own(items.size());
            for (size_t j = 0; j < items.size(); ++j) own[j] = j;
            rc = locate_subset_plan(items.data(), own.data(), items.size(), items.size(), &gs.plan);
            if (rc == KZG_OK) rc = resident_group_sums(ctx, srs, &rs, gs.plan, &gs);
            if (rc != KZG_OK) return rc;
            std::vector<uint8_t> item_ok(items.size(), 1);                               // (segment j = chosen item j)
            size_t bad_items = 0;
            rc = group_locate(ctx, true, gs, g2_tau_l, item_ok.data(), &bad_items, &level_checks);
            if (rc != KZG_OK) return rc;
            checks += level_checks;
            for (size_t j = 0; j < items.size(); ++j) if (!item_ok[j]) status[items[j]] = RETRIEVE_ITEM_BAD_EQUATION;
        }
    }
    const auto t_located = Clock::now();
    size_t bad_items = 0;
    for (size_t i = 0; i < N; ++i) bad_items += status[i] != RETRIEVE_ITEM_GOOD;
    std::vector<uint32_t> chosen;
    std::vector<uint8_t> blob_status;
    const size_t unrecovered = retrieve_choose(status.data(), blobs, count, use_count, &chosen, &blob_status);
    RecoverBatchPlan plan;
    recover_selected_plan(coset_indices, index_rows, blobs, count, use_count, chosen.data(), blob_status.data(), n, l, degree_bound, eval_form != 0, out_len,
                          ctx->recover_group_bytes, &plan);
    if (unrecovered == blobs) {                                                          // nothing to recover: zero rows, no kernel
        memset(out_polys_be, 0, blobs * plan.out_len * 32);
    } else {
        uint32_t bad_word = 0xFFFFFFFFu;                                                 // (stays: a chosen item has passed the decode, no other value is read)
        RecoverIo io;
        io.d_ys = ctx->cb[0].as<uint4>(); io.ys_be = true; io.out = out_polys_be; io.out_be = true; io.consistent = out_consistent; io.bad_word = &bad_word;
        rc = recover_run_batch(ctx, plan, io);
        if (rc != KZG_OK) return rc;
    }
    // every output is written here, behind the last call that can fail: an error leaves all of them as the caller handed them in
    // (the rows excepted, which the recovery writes group by group)
    memcpy(out_item_status, status.data(), N);
    memcpy(out_blob_status, blob_status.data(), blobs);
    *out_bad_items = bad_items;
    *out_unrecovered = unrecovered;
    if (out_pairing_checks) *out_pairing_checks = checks;
    if (out_r_powers_mont) memcpy(out_r_powers_mont, st.r_powers, N * 32);
    for (size_t b = 0; b < blobs; ++b)
        if (blob_status[b]) {                                                            // (its work row is zero already: an item map without items)
            memset(out_polys_be + b * plan.out_len * 32, 0, plan.out_len * 32);
            if (out_consistent) out_consistent[b] = 0;
        }
    if (opts().vb_trace)
        fprintf(stderr, "kzg_retrieve_blobs_bytes_tolerant blobs=%zu count=%zu use=%zu l=%zu: decode %.3f ms, r_powers%s %.3f ms, batch equation %.3f ms (%s), "
                "locate %.3f ms, %zu pairing checks, %zu bad items, %zu blobs not recovered, recover %.3f ms, call %.3f ms\n", blobs, count, use_count, l, st.ms[1],
                st.rp_path, st.ms[2], ms_between(t.start, t_verified), ok ? "holds" : "fails", ms_between(t_verified, t_located), checks, bad_items, unrecovered,
                ms_between(t_located, Clock::now()), ms_between(t0, Clock::now()));
    return KZG_OK;
}

}  // extern "C"

#if defined(KZG_DEVICE_BOUND_CHECK)
#include "field29.h"
KZG_BOUND_CHECK_EXPORTS(capi_coset)
#endif
