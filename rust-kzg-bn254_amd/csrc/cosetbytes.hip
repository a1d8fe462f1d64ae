// cosetbytes.hip — coset items decoded from their serialized form on the device: what a sampler or validator receives off the wire, 32-byte
// gnark-compressed G1 points (commitments, proofs) and 32-byte big-endian scalars (values), into the words the verifier's kernels read.
// Behind kzg_g1_decompress_be_device, kzg_coset_items_decode_be (capi_bytes.hip) and kzg_verify_multiproof_batch_bytes (capi_coset.hip).
//
//   k_g1_decode_be<WIRE>   one lane per point, 32 B in as two uint4: g1_decode.h (flags, canonical x, y = (x^3 + 3)^((p + 1) / 4) by the
//                          3-bit window of g2_decode.h, the sign rule).  Out: the device format of curve.h, 64 B, optionally twice (the
//                          fused verifier's two proof combinations are one batched MSM over concatenated bases: the kernel writes the
//                          second copy instead of a device-to-device copy behind it), or (WIRE) a wire point and its identity byte.
//                          A refused point leaves as zeros.
//   k_fr_decode_be         one lane per value, so consecutive lanes read consecutive 32-byte words: byte swap, compare with r, one product
//                          into Montgomery form.  A value >= r is refused (zeros).
//   k_mask_refused_weights one lane per item: the weight of an item whose status word is not zero becomes zero (the tolerant retriever).
// Refusals go through ONE word per array, atomicMin over index << 2 | kind, as in g2decode.hip: the reported status is that of the
// SMALLEST bad index, whatever the launch geometry.  The ITEMS instantiations (k_g1_decode_be<false, true> for the proofs, k_fr_decode_be<true>;
// kzg_retrieve_blobs_bytes_tolerant) name EVERY refused item instead: atomicOr of a COSET_ITEM_* bit into one status word per item, N words
// behind the bad words in ctx->cb[1], read with them at the one synchronisation; the commitments keep the one word.  The other
// instantiations compile as they did.  Plain vector loads and stores and those two vector atomics only; integer VALU work throughout, no
// MFMA.  The compiler's figures for the kernels: profiles/coset_bytes.md, profiles/retrieve_tolerant.md.
#include "engine.h"
#include "byte_stager.h"
#include "g1_decode.h"

#include <algorithm>
#include <string>

namespace kzg {

// ITEMS (the tolerant retriever, kzg_retrieve_blobs_bytes_tolerant): a refusal ORs its COSET_ITEM_* bit into the status word of its ITEM
// (point first + i; value (first + i) >> log_per_item) in place of the atomicMin on `bad`: every refused item is named, not the smallest
// only.  A vector atomic OR of a constant bit: the l value lanes of an item and its proof lane may meet in one word in any order.
template <bool WIRE, bool ITEMS = false>
__global__ void __launch_bounds__(256)
k_g1_decode_be(const uint4* __restrict__ bytes, uint4* __restrict__ out, uint4* __restrict__ out_copy, uint8_t* __restrict__ out_inf, uint32_t n, uint32_t first,
               uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 q0 = bytes[2 * (size_t)i], q1 = bytes[2 * (size_t)i + 1];
    const uint32_t raw[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    Fq x, y;
    const uint32_t kind = g1_decompress_point(x, y, raw);
    uint32_t o[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) o[j] = 0;
    if (kind == G1_DECODE_OK) {
        if (WIRE) g1_point_to_wire_words(o, x, y);
        else g1_point_to_device_words(o, x, y);
    } else if (kind != G1_DECODE_IDENTITY) {
        if (ITEMS) atomicOr(bad + first + i, kind == G1_BAD_NOT_ON_CURVE ? COSET_ITEM_PROOF_OFF_CURVE : COSET_ITEM_PROOF_BYTES);   // bad: the n_points status words
        else atomicMin(bad, (first + i) << 2 | kind);               // first + i < 2^28
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) out[4 * (size_t)i + k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    if (out_copy) {
#pragma unroll
        for (int k = 0; k < 4; ++k) out_copy[4 * (size_t)i + k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    }
    if (WIRE) out_inf[i] = kind == G1_DECODE_OK ? 0 : 1;
}

template <bool ITEMS = false>
__global__ void __launch_bounds__(256)
k_fr_decode_be(const uint4* __restrict__ bytes, uint4* __restrict__ out, uint32_t n, uint32_t first, uint32_t* __restrict__ bad, int log_per_item) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 q0 = bytes[2 * (size_t)i], q1 = bytes[2 * (size_t)i + 1];
    const uint32_t raw[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    uint32_t o[8];
    if (!fr_decode_be_to_wire(o, raw)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = 0;
        if (ITEMS) atomicOr(bad + ((first + i) >> log_per_item), COSET_ITEM_VALUE);   // bad: the status words, one per item of 2^log_per_item values
        else atomicMin(bad, (first + i) << 2);                      // first + i < 2^28; the one kind
    }
    out[2 * (size_t)i] = make_uint4(o[0], o[1], o[2], o[3]);
    out[2 * (size_t)i + 1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// weights[i] = 0 where item i was refused by the decode (status word not zero): the item then enters every sum of the batch equation with weight 0
__global__ void __launch_bounds__(256)
k_mask_refused_weights(uint4* __restrict__ weights, const uint32_t* __restrict__ status, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || status[i] == 0u) return;
    weights[2 * (size_t)i] = make_uint4(0, 0, 0, 0);
    weights[2 * (size_t)i + 1] = make_uint4(0, 0, 0, 0);
}

// -------------------------------------------------------------------------------------------------
// host driver (slot 0's workspace and stream)
// -------------------------------------------------------------------------------------------------
// The bytes go up through a ByteStager (byte_stager.h: the pinned halves and their lifetime rules): ONE stager serves the arrays of a
// call one after the other, the caller's own when it has staged bytes already.  A kernel starts behind every COSET_BYTES_LAUNCH bytes.
constexpr size_t COSET_BYTES_LAUNCH = 4 * STAGE_CHUNK_BYTES;        // bytes per kernel launch: 131 072 lanes

int32_t coset_bytes_enqueue(kzg_ctx* ctx, CosetBytesDecode* job, ByteStager* in_use) {
    MsmWorkspace& ws = ctx->msm;
    hipStream_t st = ctx->stream;
    const size_t M = job->n_points[0], N = job->n_points[1], V = job->n_values;
    if (M > ((size_t)1 << 28) || N > ((size_t)1 << 28) || V > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    KZG_HIP_TRY(ctx, ctx->cb[0].reserve(std::max<size_t>(V * 32, 32)));
    const bool items = job->item_status;                            // N status words behind the bad words
    KZG_HIP_TRY(ctx, ctx->cb[1].reserve((M + N) * 32 + 16 + (items ? N * 4 : 0)));
    { const int32_t rc = msm_pinned_out(ctx, ws); if (rc != KZG_OK) return rc; }
    char* d_pts = ctx->cb[1].as<char>();
    uint32_t* d_bad = reinterpret_cast<uint32_t*>(d_pts + (M + N) * 32);
    job->d_points_be[0] = reinterpret_cast<const uint4*>(d_pts);
    job->d_points_be[1] = reinterpret_cast<const uint4*>(d_pts + M * 32);
    job->d_ys_be = ctx->cb[0].as<uint4>();
    ByteStager own;
    ByteStager& stager = in_use ? *in_use : own;
    hipError_t e = in_use ? hipSuccess : own.init(st, ws.pinned_out);
    if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0xFF, 16, st);
    job->d_status = items ? d_bad + 4 : nullptr;
    if (e == hipSuccess && items && N) e = hipMemsetAsync(job->d_status, 0, N * 4, st);
    const int log_per_item = __builtin_ctzll(std::max<size_t>(job->values_per_item, 1));
    for (int a = 0; a < 2 && e == hipSuccess; ++a) {
        const size_t n = job->n_points[a];
        if (n == 0) continue;
        char* d_bytes = d_pts + (a ? M * 32 : 0);
        e = stager.push(job->points_be[a], n * 32, d_bytes, COSET_BYTES_LAUNCH, [&](size_t lo, size_t hi) {
            const size_t p0 = lo / 32;
            const uint32_t cnt = (uint32_t)((hi - lo) / 32);
            const dim3 grid((cnt + 255) / 256), block(256);
            const uint4* src = reinterpret_cast<const uint4*>(d_bytes + lo);
            uint4* copy = job->d_points_copy[a] ? job->d_points_copy[a] + 4 * p0 : nullptr;
            if (items && a == 1)
                hipLaunchKernelGGL((k_g1_decode_be<false, true>), grid, block, 0, st, src, job->d_points[a] + 4 * p0, copy, static_cast<uint8_t*>(nullptr), cnt, (uint32_t)p0, job->d_status);
            else if (job->wire_points)
                hipLaunchKernelGGL(k_g1_decode_be<true>, grid, block, 0, st, src, job->d_points[a] + 4 * p0, copy, job->d_inf[a] + p0, cnt, (uint32_t)p0, d_bad + a);
            else
                hipLaunchKernelGGL(k_g1_decode_be<false>, grid, block, 0, st, src, job->d_points[a] + 4 * p0, copy, static_cast<uint8_t*>(nullptr), cnt, (uint32_t)p0, d_bad + a);
        });
    }
    if (e == hipSuccess && V) {
        char* d_bytes = ctx->cb[0].as<char>();
        e = stager.push(job->ys_be, V * 32, d_bytes, COSET_BYTES_LAUNCH, [&](size_t lo, size_t hi) {
            const size_t v0 = lo / 32;
            const uint32_t cnt = (uint32_t)((hi - lo) / 32);
            const uint4* src = reinterpret_cast<const uint4*>(d_bytes + lo);
            if (items) hipLaunchKernelGGL(k_fr_decode_be<true>, dim3((cnt + 255) / 256), dim3(256), 0, st, src, job->d_ys + 2 * v0, cnt, (uint32_t)v0, job->d_status, log_per_item);
            else hipLaunchKernelGGL(k_fr_decode_be<false>, dim3((cnt + 255) / 256), dim3(256), 0, st, src, job->d_ys + 2 * v0, cnt, (uint32_t)v0, d_bad + 2, 0);
        });
    }
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);                             // (byte_stager.h: drained before an error leaves)
        return set_error(ctx, e, "decoding serialized coset items");
    }
    return KZG_OK;
}

int32_t coset_bytes_collect(kzg_ctx* ctx, CosetBytesDecode* job) {
    const uint32_t* d_bad = reinterpret_cast<const uint32_t*>(ctx->cb[1].as<char>() + (job->n_points[0] + job->n_points[1]) * 32);
    uint32_t h_bad[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    hipError_t e = hipMemcpyAsync(h_bad, d_bad, 12, hipMemcpyDeviceToHost, ctx->stream);
    if (job->item_status) {
        job->status.assign(job->n_points[1], 0);
        if (e == hipSuccess && job->n_points[1]) e = hipMemcpyAsync(job->status.data(), job->d_status, job->n_points[1] * 4, hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return set_error(ctx, e, "decoding serialized coset items");
    for (int a = 0; a < 3; ++a) job->bad[a] = h_bad[a];
    return KZG_OK;
}

int32_t coset_bytes_status(kzg_ctx* ctx, const char* who, const char* array, uint32_t bad_word, size_t per_item, uint64_t* bad_index) {
    if (bad_word == 0xFFFFFFFFu) return KZG_OK;
    const size_t index = (bad_word >> 2) / per_item;
    const bool off_curve = (bad_word & 3u) == G1_BAD_NOT_ON_CURVE;
    if (bad_index) *bad_index = index;
    ctx->last_error = std::string(who) + ": " + array + " " + std::to_string(index) +
                      (off_curve ? " has no point on the curve" : " is not a canonical encoding (flag bits, or an integer not below the modulus)");
    return off_curve ? KZG_ERR_NOT_ON_CURVE : KZG_ERR_DESERIALIZE;
}

int32_t coset_mask_refused_weights(kzg_ctx* ctx, uint4* d_weights, const uint32_t* d_status, size_t count) {
    if (count == 0) return KZG_OK;
    hipLaunchKernelGGL(k_mask_refused_weights, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, d_weights, d_status, (uint32_t)count);
    KZG_HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

}  // namespace kzg

KZG_BOUND_CHECK_EXPORTS(cosetbytes)
