// headerbytes.hip — blob headers decoded from their serialized form on the device: what a validator receives off the wire, per header a
// 32-byte gnark-compressed commitment (g1_decode.h) and two 64-byte gnark-compressed G2 elements from an untrusted disperser (g2_decode.h),
// into the words the header-batch kernels read.  Behind kzg_header_items_decode_be, kzg_verify_length_proof_batch_bytes and
// kzg_verify_length_proof_batch_locate_bytes (capi_g2.hip).
//
//   k_header_g2_decode<WIRE>   one lane per G2 element (element 2 i = C2_i, 2 i + 1 = pi2_i, read from the two byte arrays): the identity
//                              rule of the header format (0x40 || 63 zero bytes; 0b01 with any other bit set is refused), else
//                              g2_decompress_point and the order-r subgroup test g2_in_subgroup, fused as in k_g2_decompress: the one
//                              63-bit chain an element gets.  The generator is a valid element.  Out: the device format of curve_g2.h in
//                              the order the chains read (C2_0, pi2_0, C2_1, ..), or (WIRE) wire points, every C2 in front of every pi2;
//                              the identity and a refused element as zeros.  One atomicMin of element << 2 | kind keeps the SMALLEST bad
//                              element with its own kind: the smallest header, C2 in front of pi2, whatever the launch geometry.
//                              The budget is k_g2_decompress's: one wave per SIMD, one element per lane.
//   k_header_item_digests      one lane per header: the 320-byte item message of the header transcript, block by block in registers
//                              (header_item_stream.h: the commitment's bytes as they arrived, the G2 elements from the decoded points
//                              where the chains read them), six SHA-256 compressions.  A workgroup is one wave, as in fsdevice.hip.
// The commitments go through k_g1_decode_be (cosetbytes.hip).  Plain vector loads and stores only; integer VALU work throughout, no MFMA.
// The compiler's figures for the kernels and the measured times: profiles/header_bytes.md.
#include "engine.h"
#include "byte_stager.h"
#include "g2_decode.h"
#include "header_item_stream.h"

#include <algorithm>
#include <string>

namespace kzg {

// c2 / pi2: the two byte arrays of the whole batch; the launch covers the elements of headers [h0, h0 + n_elems / 2)
template <bool WIRE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_header_g2_decode(const uint4* __restrict__ c2, const uint4* __restrict__ pi2, uint4* __restrict__ out, uint32_t n_elems, uint32_t h0, uint32_t count,
                   uint32_t* __restrict__ bad) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_elems) return;
    const uint32_t h = h0 + (e >> 1), which = e & 1u;
    if (h >= count) return;
    uint32_t raw[16];
    g2_load_raw(raw, (which ? pi2 : c2) + 4 * (size_t)h);
    uint32_t rest = raw[0] ^ 0x40u;                                 // the identity: byte 0 = 0x40, every other bit zero
#pragma unroll
    for (int k = 1; k < 16; ++k) rest |= raw[k];
    const bool identity = rest == 0;
    G2Affine p;
    uint32_t kind = G2_DECODE_OK;
    if (!identity) {
        kind = g2_decompress_point(p, raw);                         // (flags 0b00 and 0b01 leave here as G2_BAD_DESERIALIZE)
        if (kind == G2_DECODE_OK && !g2_in_subgroup(p)) kind = G2_BAD_SUBGROUP;
    }
    uint32_t o[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) o[j] = 0;
    if (kind != G2_DECODE_OK) atomicMin(bad, (2 * h + which) << 2 | kind);      // 2 h + which < 2^21
    else if (!identity) g2_point_to_words<WIRE>(o, p);
    g2_store_words(out + 8 * (WIRE ? (size_t)which * count + h : 2 * (size_t)h + which), o);
}

constexpr uint32_t HEADER_FS_LANES = 64;

// commitments_be: 32 B per header as they arrived; g2: the device-format points C2_0, pi2_0, C2_1, ..; out: 32 B per header
__global__ void __launch_bounds__(HEADER_FS_LANES)
k_header_item_digests(const uint4* __restrict__ commitments_be, const uint4* __restrict__ g2, const uint64_t* __restrict__ claimed_lens, uint32_t count,
                      uint4* __restrict__ out) {
    const uint32_t i = blockIdx.x * HEADER_FS_LANES + threadIdx.x;
    if (i >= count) return;
    HeaderItemSrc src;
    src.commitment_be = reinterpret_cast<const uint32_t*>(commitments_be + 2 * (size_t)i);
    src.c2 = reinterpret_cast<const uint32_t*>(g2 + 16 * (size_t)i);
    src.pi2 = reinterpret_cast<const uint32_t*>(g2 + 16 * (size_t)i + 8);
    src.d = claimed_lens[i];
    uint32_t o[8];
    header_item_digest(o, src);
    out[2 * (size_t)i] = make_uint4(o[0], o[1], o[2], o[3]);
    out[2 * (size_t)i + 1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// -------------------------------------------------------------------------------------------------
// host drivers (slot 0's workspace and stream, synchronised on return)
// -------------------------------------------------------------------------------------------------
// ONE ByteStager (byte_stager.h: the pinned halves and their lifetime rules) serves the whole call: per run of HEADER_PIECE headers a piece
// of C2 bytes and a piece of pi2 bytes, a kernel behind every HEADER_DECODE_LAUNCH headers, then the commitments through
// coset_bytes_enqueue (cosetbytes.hip) on the same stager, whose wait-before-reuse covers the halves the last G2 pieces are leaving.
constexpr size_t HEADER_PIECE = STAGE_CHUNK_BYTES / 64;              // headers per staged piece of either G2 array
constexpr size_t HEADER_DECODE_LAUNCH = 2 * HEADER_PIECE;            // headers per launch of k_header_g2_decode: 65 536 lanes

int32_t header_bytes_decode(kzg_ctx* ctx, HeaderBytesDecode* job) {
    const size_t n = job->count;
    job->bad_g1 = job->bad_g2 = 0xFFFFFFFFu;
    if (n == 0) return KZG_OK;
    if (n > ((size_t)1 << 20)) return KZG_ERR_TOO_LARGE;
    MsmWorkspace& ws = ctx->msm;
    hipStream_t st = ctx->stream;
    KZG_HIP_TRY(ctx, ws.bases_wire.reserve(2 * n * 64 + 16));
    { const int32_t rc = msm_pinned_out(ctx, ws); if (rc != KZG_OK) return rc; }
    char* d_arr[2] = {ws.bases_wire.as<char>(), ws.bases_wire.as<char>() + n * 64};
    uint32_t* d_bad = reinterpret_cast<uint32_t*>(ws.bases_wire.as<char>() + 2 * n * 64);
    const uint8_t* h_arr[2] = {job->length_commitments_be, job->length_proofs_be};
    ByteStager stager;
    hipError_t e = stager.init(st, ws.pinned_out);
    if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0xFF, 4, st);
    size_t launched = 0;
    for (size_t lo = 0; lo < n && e == hipSuccess; lo += HEADER_PIECE) {
        const size_t len = std::min(HEADER_PIECE, n - lo);
        for (int a = 0; a < 2 && e == hipSuccess; ++a) e = stager.copy(h_arr[a] + lo * 64, len * 64, d_arr[a] + lo * 64);
        const size_t staged = lo + len;
        if (e == hipSuccess && (staged - launched >= HEADER_DECODE_LAUNCH || staged == n)) {
            const uint32_t cnt = (uint32_t)(2 * (staged - launched));
            const dim3 grid((cnt + 255) / 256), block(256);
            const uint4 *c2 = reinterpret_cast<const uint4*>(d_arr[0]), *pi2 = reinterpret_cast<const uint4*>(d_arr[1]);
            if (job->wire) hipLaunchKernelGGL(k_header_g2_decode<true>, grid, block, 0, st, c2, pi2, job->d_g2, cnt, (uint32_t)launched, (uint32_t)n, d_bad);
            else hipLaunchKernelGGL(k_header_g2_decode<false>, grid, block, 0, st, c2, pi2, job->d_g2, cnt, (uint32_t)launched, (uint32_t)n, d_bad);
            e = hipGetLastError();
            launched = staged;
        }
    }
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);                                                    // (byte_stager.h: drained before an error leaves)
        return set_error(ctx, e, "decoding serialized header elements");
    }
    CosetBytesDecode g1;
    g1.points_be[0] = job->commitments_be;
    g1.n_points[0] = n;
    g1.d_points[0] = job->d_commitments;
    g1.d_inf[0] = job->d_commitments_inf;
    g1.wire_points = job->wire;
    int32_t rc = coset_bytes_enqueue(ctx, &g1, &stager);
    uint32_t h_bad = 0xFFFFFFFFu;
    if (rc == KZG_OK) e = hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st);
    const int32_t rc2 = rc == KZG_OK ? coset_bytes_collect(ctx, &g1) : ((void)hipStreamSynchronize(st), rc);     // (drains the stream on every path)
    if (rc2 != KZG_OK) return rc2;
    if (e != hipSuccess) return set_error(ctx, e, "decoding serialized header elements");
    job->d_commitments_be = g1.d_points_be[0];
    job->bad_g1 = g1.bad[0];
    job->bad_g2 = h_bad;
    return KZG_OK;
}

int32_t header_bytes_status(kzg_ctx* ctx, const char* who, const HeaderBytesDecode& job, uint64_t* bad_index, int32_t* bad_array) {
    int32_t rc = coset_bytes_status(ctx, who, "commitment", job.bad_g1, 1, bad_index);
    if (rc != KZG_OK) { if (bad_array) *bad_array = 0; return rc; }
    if (job.bad_g2 == 0xFFFFFFFFu) return KZG_OK;
    static const char* const what[3] = {"is not a canonical encoding (flag bits, or a coordinate not below the modulus)", "has no point on the twist",
                                        "is not in the order-r subgroup"};
    const uint32_t elem = job.bad_g2 >> 2, kind = job.bad_g2 & 3u;
    if (bad_index) *bad_index = elem >> 1;
    if (bad_array) *bad_array = 1 + (int32_t)(elem & 1u);
    ctx->last_error = std::string(who) + ": the length " + (elem & 1u ? "proof" : "commitment") + " of header " + std::to_string(elem >> 1) + " " + what[kind < 3 ? kind : 2];
    return kind == G2_BAD_DESERIALIZE ? KZG_ERR_DESERIALIZE : KZG_ERR_NOT_ON_CURVE;
}

int32_t header_item_digests_run(kzg_ctx* ctx, const uint4* d_commitments_be, const uint4* d_g2, const uint64_t* claimed_lens, size_t count, uint8_t* out_digests) {
    if (count == 0) return KZG_OK;
    hipStream_t st = ctx->stream;
    KZG_HIP_TRY(ctx, ctx->fs[0].reserve(count * 8 + 16));
    KZG_HIP_TRY(ctx, ctx->fs[1].reserve(count * 32));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->fs[0].p, claimed_lens, count * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_header_item_digests, dim3((unsigned)((count + HEADER_FS_LANES - 1) / HEADER_FS_LANES)), dim3(HEADER_FS_LANES), 0, st, d_commitments_be, d_g2,
                       ctx->fs[0].as<uint64_t>(), (uint32_t)count, ctx->fs[1].as<uint4>());
    KZG_HIP_TRY(ctx, hipGetLastError());
    KZG_HIP_TRY(ctx, hipMemcpyAsync(out_digests, ctx->fs[1].p, count * 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return KZG_OK;
}

}  // namespace kzg

KZG_BOUND_CHECK_EXPORTS(headerbytes)
