// capi_provebatch.hip -- the C-ABI of the batched prover: kzg_compute_proof_batch(_device), kzg_compute_blob_proof_batch,
// kzg_commit_and_prove_blob_batch, kzg_ctx_set_prove_group_bytes.  host_prove_batch.h checks and plans (length classes, groups under the
// context's byte budget, packing, scatter); provebatch.hip runs a group: rows on the device, [commitments], [transcripts on the host pool],
// the fused evaluate-and-divide kernel, the quotient rows' commitments over the cached Lagrange basis.  Blobs of more than 2^12 elements take
// the single-proof path inside the call.
#include "engine.h"
#include "host_curve.h"
#include "host_pairing.h"
#include "host_sha256.h"
#include "host_fiat_shamir.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

using namespace kzg;

namespace {
// the batched MSM runs on the slots' streams and workspaces: nothing may be in flight on any of them (as for kzg_commit_*_batch)
bool any_slot_pending(kzg_ctx* ctx) {
    for (int sl = 0; sl < KZG_NUM_SLOTS; ++sl)
        if (ctx->slot_pending[sl]) {
            ctx->last_error = "a kzg_*_begin is still in flight: the batched prover uses the slots' streams and workspaces itself";
            return true;
        }
    return false;
}

// the cached Lagrange basis of n points, attached to the SRS on first use (takes ctx->mu itself: call it before the lock)
int32_t lagrange_basis(kzg_ctx* ctx, kzg_srs* srs, size_t n, kzg_srs** out) {
    int32_t rc = kzg_srs_cache_lagrange(ctx, srs, n);
    if (rc != KZG_OK) return rc;
    *out = srs_cached_lagrange(srs, n);
    return *out ? KZG_OK : KZG_ERR_INVALID_ARG;               // dropped by another thread between the two calls
}

int32_t proof_batch_common(kzg_ctx* ctx, kzg_srs* srs, const void* evals, bool on_device, size_t n, size_t count, const uint64_t* zs,
                           uint64_t* out_xy, uint8_t* out_inf, uint64_t* out_ys) {
    bool done = false;
    const bool bad_handles = !ctx || !srs || srs->ctx != ctx || !out_xy;
    int32_t rc = prove_batch_check_polys(bad_handles, !evals || !zs, n, count, bad_handles ? 0 : srs->n, &done);
    if (rc != KZG_OK || done) return rc;
    const uint64_t* h_evals = static_cast<const uint64_t*>(evals);
    if (n > ((size_t)1 << PROVE_BATCH_MAX_LOG)) {             // the single-proof path, one polynomial after the other
        std::lock_guard<std::mutex> lk(ctx->mu);
        KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (any_slot_pending(ctx)) return KZG_ERR_INVALID_ARG;
        for (size_t b = 0; b < count; ++b) {
            if (on_device) {                                  // proof_run takes resident evaluations in slot 0's buffer
                KZG_HIP_TRY(ctx, ctx->poly[0].a.reserve(n * 32 + 32));
                KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->poly[0].a.p, static_cast<const char*>(evals) + b * n * 32, n * 32, hipMemcpyDeviceToDevice, ctx->stream));
            }
            rc = proof_run(ctx, srs, on_device ? nullptr : h_evals + 4 * b * n, n, zs + 4 * b, out_xy + 8 * b, out_inf ? out_inf + b : nullptr,
                           out_ys ? out_ys + 4 * b : nullptr, true, 0, nullptr);
            if (rc != KZG_OK) return rc;
        }
        return KZG_OK;
    }
    kzg_srs* basis = nullptr;
    rc = lagrange_basis(ctx, srs, n, &basis);
    if (rc != KZG_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (any_slot_pending(ctx)) return KZG_ERR_INVALID_ARG;
    const int log_n = prove_batch_log2(n);
    const size_t group = prove_batch_group_rows(n, count, ctx->prove_group_bytes, false);
    for (size_t g0 = 0; g0 < count; g0 += group) {
        const size_t rows = std::min(group, count - g0);
        const void* d_rows = static_cast<const char*>(evals) + g0 * n * 32;
        if (!on_device) {
            KZG_HIP_TRY(ctx, ctx->pb[1].reserve(rows * n * 32 + 32));
            KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->pb[1].p, h_evals + 4 * g0 * n, rows * n * 32, hipMemcpyHostToDevice, ctx->stream));
            d_rows = ctx->pb[1].p;
        }
        rc = prove_batch_rows_run(ctx, basis, d_rows, log_n, rows, zs + 4 * g0, out_xy + 8 * g0, out_inf ? out_inf + g0 : nullptr, out_ys ? out_ys + 4 * g0 : nullptr);
        if (rc != KZG_OK) return rc;
    }
    return KZG_OK;
}

// commitments_in given: kzg_compute_blob_proof per blob; else kzg_commit_and_prove_blob per blob, the commitments into out_commitments
int32_t blob_proof_batch_common(kzg_ctx* ctx, kzg_srs* srs, const uint8_t* const* blobs, const size_t* lens, const uint64_t* commitments_in, bool commit, size_t count,
                                uint64_t* out_commitments, uint8_t* out_commitment_inf, uint64_t* out_proofs, uint8_t* out_inf, uint64_t* out_zs, uint64_t* out_ys,
                                size_t* out_bad_index) {
    using namespace kzg_host;
    if (!ctx || !srs || srs->ctx != ctx || !out_proofs || (commit && !out_commitments)) return KZG_ERR_INVALID_ARG;
    if (count == 0) return KZG_OK;
    if (!blobs || !lens || (!commit && !commitments_in)) return KZG_ERR_INVALID_ARG;
    // every blob's status in the single call's order, then the first failing one in index order
    std::vector<int32_t> status(count);
    {
        auto one = [&](size_t i) {
            const bool off_curve = !commit && !g1_on_curve(g1_from_wire(commitments_in + 8 * i));
            status[i] = prove_batch_blob_status(blobs[i] == nullptr, lens[i], off_curve, srs->n);
        };
        if (!commit && count >= 256) host_parallel_for(count, one);
        else for (size_t i = 0; i < count; ++i) one(i);
    }
    int32_t rc = prove_batch_first_failure(status.data(), count, out_bad_index);
    if (rc != KZG_OK) return rc;
    const ProveBatchPlan plan = prove_batch_plan(lens, count);
    std::vector<kzg_srs*> bases(plan.classes.size(), nullptr);
    for (size_t c = 0; c < plan.classes.size(); ++c) {
        rc = lagrange_basis(ctx, srs, (size_t)1 << plan.classes[c].log_n, &bases[c]);
        if (rc != KZG_OK) return rc;
    }
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (any_slot_pending(ctx)) return KZG_ERR_INVALID_ARG;
        const bool trace = opts().vb_trace != 0;
        std::vector<size_t> offs;
        std::vector<VbBlob> meta;
        std::vector<Sha256> hashes;
        std::vector<uint64_t> g_cm, g_pr, g_zs, g_ys;
        std::vector<uint8_t> g_cinf, g_inf;
        for (size_t c = 0; c < plan.classes.size(); ++c) {
            const ProveBatchClass& cls = plan.classes[c];
            const size_t n = (size_t)1 << cls.log_n;
            const size_t group = prove_batch_group_rows(n, cls.count, ctx->prove_group_bytes, true);
            for (size_t g0 = 0; g0 < cls.count; g0 += group) {
                const size_t rows = std::min(group, cls.count - g0);
                const size_t* order = plan.order.data() + cls.first + g0;
                offs.resize(rows + 1);
                prove_batch_pack_offsets(lens, order, rows, offs.data());
                const size_t packed_bytes = offs[rows];
                if (packed_bytes + 4096 > ctx->vb_pinned_bytes) {           // the pinned staging of the batch verifier: the same packed form
                    if (ctx->vb_pinned) { (void)hipHostFree(ctx->vb_pinned); ctx->vb_pinned = nullptr; ctx->vb_pinned_bytes = 0; }
                    const size_t cap = packed_bytes + packed_bytes / 4 + 8192;
                    KZG_HIP_TRY(ctx, hipHostMalloc(&ctx->vb_pinned, cap, hipHostMallocDefault));
                    ctx->vb_pinned_bytes = cap;
                }
                uint8_t* stage = static_cast<uint8_t*>(ctx->vb_pinned);
                meta.resize(rows);
                const auto t0 = Clock::now();
                host_parallel_for(rows, [&](size_t r) {                      // pack: the blob, zeros up to its last whole element
                    const size_t i = order[r], span = offs[r + 1] - offs[r];
                    memcpy(stage + offs[r], blobs[i], lens[i]);
                    if (span > lens[i]) memset(stage + offs[r] + lens[i], 0, span - lens[i]);
                    meta[r] = VbBlob{(uint64_t)offs[r], (uint32_t)lens[i], (uint32_t)cls.log_n};
                });
                const void* d_rows = nullptr;
                rc = prove_batch_rows_from_bytes(ctx, stage, packed_bytes, meta.data(), rows, cls.log_n, &d_rows);   // upload and bytes -> Fr run beside the hashing
                if (rc != KZG_OK) return rc;
                hashes.resize(rows);
                g_zs.resize(rows * 4);
                host_parallel_for(rows, [&](size_t r) {                      // transcripts: exactly compute_challenge's bytes (helpers.rs:411-455)
                    const size_t i = order[r];
                    sha256_init(hashes[r]);
                    challenge_absorb_prefix(hashes[r], stage + offs[r], lens[i], n);
                    if (!commit) challenge_finish(hashes[r], g1_from_wire(commitments_in + 8 * i), g_zs.data() + 4 * r);
                });
                const auto t1 = Clock::now();
                KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));         // the rows are complete (and the staging buffer is free again)
                if (commit) {
                    g_cm.resize(rows * 8);
                    g_cinf.resize(rows);
                    rc = commit_batch_device(ctx, bases[c], d_rows, n, rows, g_cm.data(), g_cinf.data());   // kzg.rs:182-185 over the Lagrange basis
                    if (rc != KZG_OK) return rc;
                    host_parallel_for(rows, [&](size_t r) { challenge_finish(hashes[r], g1_from_wire(g_cm.data() + 8 * r), g_zs.data() + 4 * r); });
                    prove_batch_scatter(g_cm.data(), order, rows, 8, out_commitments);
                    prove_batch_scatter_bytes(g_cinf.data(), order, rows, out_commitment_inf);
                }
                const auto t2 = Clock::now();
                g_pr.resize(rows * 8);
                g_inf.resize(rows);
                g_ys.resize(rows * 4);
                rc = prove_batch_rows_run(ctx, bases[c], d_rows, cls.log_n, rows, g_zs.data(), g_pr.data(), g_inf.data(), out_ys ? g_ys.data() : nullptr);
                if (rc != KZG_OK) return rc;
                prove_batch_scatter(g_pr.data(), order, rows, 8, out_proofs);
                prove_batch_scatter_bytes(g_inf.data(), order, rows, out_inf);
                prove_batch_scatter(g_zs.data(), order, rows, 4, out_zs);
                prove_batch_scatter(g_ys.data(), order, rows, 4, out_ys);
                if (trace)
                    fprintf(stderr, "  blob_proof_batch n=%zu rows=%zu (%zu packed bytes): pack + upload + transcripts %.3f ms, commitments + challenges %.3f ms, proofs %.3f ms\n", n,
                            rows, packed_bytes, ms_between(t0, t1), ms_between(t1, t2), ms_between(t2, Clock::now()));
            }
        }
    }
    // more than 2^12 elements: the single calls, whose roots are the blob's own padded length (they take the lock themselves)
    for (size_t i : plan.single) {
        const size_t n = blob_padded_len(lens[i]);
        uint8_t* inf = out_inf ? out_inf + i : nullptr;
        uint64_t* z = out_zs ? out_zs + 4 * i : nullptr;
        uint64_t* y = out_ys ? out_ys + 4 * i : nullptr;
        if (commit)
            rc = kzg_commit_and_prove_blob(ctx, srs, blobs[i], lens[i], n, out_commitments + 8 * i, out_commitment_inf ? out_commitment_inf + i : nullptr, out_proofs + 8 * i,
                                           inf, z, y);
        else
            rc = kzg_compute_blob_proof(ctx, srs, blobs[i], lens[i], n, commitments_in + 8 * i, out_proofs + 8 * i, inf, z, y);
        if (rc != KZG_OK) { if (out_bad_index) *out_bad_index = i; return rc; }
    }
    return KZG_OK;
}
}  // namespace

extern "C" {

int32_t kzg_compute_proof_batch(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* evals_mont, size_t n, size_t count, const uint64_t* zs_mont,
                                uint64_t* out_proofs_xy_mont, uint8_t* out_is_infinity, uint64_t* out_ys_mont) {
    return proof_batch_common(ctx, srs, evals_mont, false, n, count, zs_mont, out_proofs_xy_mont, out_is_infinity, out_ys_mont);
}
int32_t kzg_compute_proof_batch_device(kzg_ctx* ctx, kzg_srs* srs, const void* d_evals_mont, size_t n, size_t count, const uint64_t* zs_mont,
                                       uint64_t* out_proofs_xy_mont, uint8_t* out_is_infinity, uint64_t* out_ys_mont) {
    return proof_batch_common(ctx, srs, d_evals_mont, true, n, count, zs_mont, out_proofs_xy_mont, out_is_infinity, out_ys_mont);
}

int32_t kzg_compute_blob_proof_batch(kzg_ctx* ctx, kzg_srs* srs, const uint8_t* const* blobs, const size_t* blob_lens, const uint64_t* commitments_xy_mont,
                                     size_t count, uint64_t* out_proofs_xy_mont, uint8_t* out_is_infinity, uint64_t* out_zs_mont, uint64_t* out_ys_mont,
                                     size_t* out_bad_index) {
    return blob_proof_batch_common(ctx, srs, blobs, blob_lens, commitments_xy_mont, false, count, nullptr, nullptr, out_proofs_xy_mont, out_is_infinity, out_zs_mont,
                                   out_ys_mont, out_bad_index);
}

int32_t kzg_commit_and_prove_blob_batch(kzg_ctx* ctx, kzg_srs* srs, const uint8_t* const* blobs, const size_t* blob_lens, size_t count,
                                        uint64_t* out_commitments_xy_mont, uint8_t* out_commitment_is_infinity, uint64_t* out_proofs_xy_mont,
                                        uint8_t* out_proof_is_infinity, uint64_t* out_zs_mont, uint64_t* out_ys_mont, size_t* out_bad_index) {
    return blob_proof_batch_common(ctx, srs, blobs, blob_lens, nullptr, true, count, out_commitments_xy_mont, out_commitment_is_infinity, out_proofs_xy_mont,
                                   out_proof_is_infinity, out_zs_mont, out_ys_mont, out_bad_index);
}

int32_t kzg_ctx_set_prove_group_bytes(kzg_ctx* ctx, size_t bytes) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->prove_group_bytes = bytes;
    return KZG_OK;
}

}  // extern "C"

#if defined(KZG_DEVICE_BOUND_CHECK)
#include "field29.h"
KZG_BOUND_CHECK_EXPORTS(capi_provebatch)
#endif
