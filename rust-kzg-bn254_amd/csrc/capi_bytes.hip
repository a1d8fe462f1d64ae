// capi_bytes.hip — the serialized-form surface of the C-ABI: gnark-compressed G1 points and big-endian scalars to and from the wire words the
// verifier entries take (cosetbytes.hip on the device, host_coset_bytes.h on the host).  The fused verifier, kzg_verify_multiproof_batch_bytes,
// lives beside the entry it mirrors in capi_coset.hip, and so does the retriever's call built on it, kzg_retrieve_blobs_bytes; the recovery with the
// codec inside, kzg_recover_from_cosets_batch_bytes, is here.
#include "engine.h"
#include "host_coset_bytes.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>

using namespace kzg;

extern "C" {

int32_t kzg_g1_decompress_be_device(kzg_ctx* ctx, const uint8_t* bytes, size_t n_points, uint64_t* out_xy_mont, uint8_t* out_is_infinity, uint64_t* bad_index) {
    if (!ctx || (n_points && (!bytes || !out_xy_mont))) return KZG_ERR_INVALID_ARG;
    if (n_points > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    if (n_points == 0) return KZG_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_refused(ctx)) return KZG_ERR_INVALID_ARG;
    KZG_HIP_TRY(ctx, ctx->msm.bases.reserve(n_points * 65));                              // wire points | identity bytes
    CosetBytesDecode job;
    job.points_be[0] = bytes;
    job.n_points[0] = n_points;
    job.d_points[0] = ctx->msm.bases.as<uint4>();
    job.d_inf[0] = ctx->msm.bases.as<uint8_t>() + n_points * 64;
    job.wire_points = true;
    int32_t rc = coset_bytes_enqueue(ctx, &job);
    if (rc == KZG_OK) rc = coset_bytes_collect(ctx, &job);
    if (rc != KZG_OK) return rc;
    rc = coset_bytes_status(ctx, "kzg_g1_decompress_be_device", "point", job.bad[0], 1, bad_index);
    if (rc != KZG_OK) return rc;
    KZG_HIP_TRY(ctx, hipMemcpyAsync(out_xy_mont, job.d_points[0], n_points * 64, hipMemcpyDeviceToHost, ctx->stream));
    if (out_is_infinity) KZG_HIP_TRY(ctx, hipMemcpyAsync(out_is_infinity, job.d_inf[0], n_points, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KZG_OK;
}

int32_t kzg_coset_items_decode_be(kzg_ctx* ctx, const uint8_t* ys_be, const uint8_t* proofs_be, size_t count, size_t chunk_len, uint64_t* out_ys_mont,
                                  uint64_t* out_proofs_xy_mont, uint64_t* bad_index, int32_t* bad_array) {
    if (!ctx || (ys_be == nullptr) != (out_ys_mont == nullptr) || (proofs_be == nullptr) != (out_proofs_xy_mont == nullptr)) return KZG_ERR_INVALID_ARG;
    if (count && !ys_be && !proofs_be) return KZG_ERR_INVALID_ARG;
    if (ys_be && chunk_len == 0) return KZG_ERR_INVALID_ARG;
    if (count > ((size_t)1 << 28) / std::max<size_t>(chunk_len, 1)) return KZG_ERR_TOO_LARGE;
    if (count == 0) return KZG_OK;
    const size_t V = ys_be ? count * chunk_len : 0, N = proofs_be ? count : 0;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_refused(ctx)) return KZG_ERR_INVALID_ARG;
    KZG_HIP_TRY(ctx, ctx->msm.bases.reserve(std::max<size_t>(N * 65, 64)));
    KZG_HIP_TRY(ctx, ctx->mv[0].reserve(std::max<size_t>(V * 32, 32)));
    CosetBytesDecode job;
    job.points_be[1] = proofs_be;
    job.n_points[1] = N;
    job.d_points[1] = ctx->msm.bases.as<uint4>();
    job.d_inf[1] = ctx->msm.bases.as<uint8_t>() + N * 64;
    job.wire_points = true;
    job.ys_be = ys_be;
    job.n_values = V;
    job.d_ys = ctx->mv[0].as<uint4>();
    int32_t rc = coset_bytes_enqueue(ctx, &job);
    if (rc == KZG_OK) rc = coset_bytes_collect(ctx, &job);
    if (rc != KZG_OK) return rc;
    rc = coset_bytes_status(ctx, "kzg_coset_items_decode_be", "proof", job.bad[1], 1, bad_index);
    if (rc != KZG_OK) { if (bad_array) *bad_array = 1; return rc; }
    rc = coset_bytes_status(ctx, "kzg_coset_items_decode_be", "value of item", job.bad[2], chunk_len, bad_index);
    if (rc != KZG_OK) { if (bad_array) *bad_array = 2; return rc; }
    if (N) KZG_HIP_TRY(ctx, hipMemcpyAsync(out_proofs_xy_mont, job.d_points[1], N * 64, hipMemcpyDeviceToHost, ctx->stream));
    if (V) KZG_HIP_TRY(ctx, hipMemcpyAsync(out_ys_mont, job.d_ys, V * 32, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KZG_OK;
}

int32_t kzg_coset_items_encode_be(const uint64_t* ys_mont, const uint64_t* proofs_xy_mont, size_t count, size_t chunk_len, uint8_t* out_ys_be, uint8_t* out_proofs_be) {
    if ((ys_mont == nullptr) != (out_ys_be == nullptr) || (proofs_xy_mont == nullptr) != (out_proofs_be == nullptr)) return KZG_ERR_INVALID_ARG;
    if (count && !ys_mont && !proofs_xy_mont) return KZG_ERR_INVALID_ARG;
    if (ys_mont && chunk_len == 0) return KZG_ERR_INVALID_ARG;
    if (count > ((size_t)1 << 28) / std::max<size_t>(chunk_len, 1)) return KZG_ERR_TOO_LARGE;
    std::atomic<int> bad{0};
    const size_t per = std::max<size_t>(1, 1024 / std::max<size_t>(chunk_len, 1)), jobs = (count + per - 1) / per;
    host_parallel_for(jobs, [&](size_t j) {
        for (size_t i = j * per; i < std::min(count, (j + 1) * per); ++i) {
            if (ys_mont)
                for (size_t t = 0; t < chunk_len; ++t)
                    if (!kzg_host::fr_encode_be(ys_mont + 4 * (i * chunk_len + t), out_ys_be + 32 * (i * chunk_len + t))) bad.store(1, std::memory_order_relaxed);
            if (proofs_xy_mont && !kzg_host::g1_encode_be(proofs_xy_mont + 8 * i, out_proofs_be + 32 * i)) bad.store(1, std::memory_order_relaxed);
        }
    });
    return bad.load() ? KZG_ERR_INVALID_ARG : KZG_OK;
}

// kzg_recover_from_cosets_batch with the codec inside the call: the values go up once as bytes and are decoded where the scatter kernel loads
// them, the rows are encoded where the last kernel stores them (recover.hip).  Checks on the host first (host_recover.h)
int32_t kzg_recover_from_cosets_batch_bytes(kzg_ctx* ctx, const uint8_t* ys_be, const uint64_t* coset_indices, size_t index_rows, size_t blobs, size_t count, size_t n,
                                            size_t chunk_len, size_t degree_bound, int32_t eval_form, size_t out_len, uint8_t* out_polys_be, int32_t* out_consistent,
                                            uint64_t* bad_index) {
    int32_t rc = recover_bytes_check(!ctx || !ys_be || !coset_indices || !out_polys_be, coset_indices, index_rows, blobs, count, n, chunk_len, degree_bound,
                                     eval_form != 0, out_len);
    if (rc != KZG_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_refused(ctx)) return KZG_ERR_INVALID_ARG;
    RecoverBatchPlan plan;
    recover_batch_plan(coset_indices, index_rows, blobs, count, n, chunk_len, degree_bound, eval_form != 0, out_len, ctx->recover_group_bytes, &plan);
    uint32_t bad_word = 0xFFFFFFFFu;
    RecoverIo io;
    io.ys = ys_be; io.ys_be = true; io.out = out_polys_be; io.out_be = true; io.consistent = out_consistent; io.bad_word = &bad_word;
    rc = recover_run_batch(ctx, plan, io);
    if (rc == KZG_ERR_DESERIALIZE) return coset_bytes_status(ctx, "kzg_recover_from_cosets_batch_bytes", "value of item", bad_word, chunk_len, bad_index);
    return rc;
}

int32_t kzg_compute_multiproof_r_powers_bytes(const uint8_t* commitments_be, size_t n_commitments, const uint64_t* commitment_indices, const uint64_t* coset_indices,
                                              const uint8_t* ys_be, const uint8_t* proofs_be, size_t count, size_t n, size_t chunk_len, uint64_t* out_r_powers_mont) {
    if (count == 0) return KZG_OK;
    if (!commitment_indices || !coset_indices || !ys_be || !proofs_be || !out_r_powers_mont || (n_commitments && !commitments_be)) return KZG_ERR_INVALID_ARG;
    if (chunk_len == 0 || count > ((size_t)1 << 28) / chunk_len) return chunk_len == 0 ? KZG_ERR_INVALID_ARG : KZG_ERR_TOO_LARGE;
    kzg_host::multiproof_r_powers_bytes_host(commitments_be, n_commitments, commitment_indices, coset_indices, ys_be, proofs_be, count, n, chunk_len, out_r_powers_mont,
                                             host_parallel_for);
    return KZG_OK;
}

}  // extern "C"

#if defined(KZG_DEVICE_BOUND_CHECK)
#include "field29.h"
KZG_BOUND_CHECK_EXPORTS(capi_bytes)
#endif
