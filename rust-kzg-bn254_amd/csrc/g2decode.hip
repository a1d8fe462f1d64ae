// g2decode.hip — gnark-compressed G2 points decoded on the device (g2_decode.h): kzg_g2_decompress_be_device and
// kzg_g2srs_load_compressed_be of the C-ABI (capi_g2.hip).  The host decoder (host_g2_decode.h, kzg_g2_decompress_be) stays as the
// yardstick; it costs about a millisecond per point and thread.
//
//   k_g2_decompress<WIRE>   one lane per point: byte decode, y = sqrt(x^3 + b) with two exponentiations, the sign rule, then the optional
//                           order-r subgroup test (g2_in_subgroup, the 63-bit chain of g2_chain.h) and the optional "not the generator";
//                           the point leaves in the device format of a kzg_g2srs (WIRE = false) or as wire words (WIRE = true), a
//                           refused point as zeros.  One atomicMin of index << 2 | kind keeps the SMALLEST bad index with its own kind
//                           (the host decoder's contract is the first bad point in file order, not the first lane to arrive).
// Square root and chain are ONE kernel: the square root's values are dead when the chain starts, so the register need is the larger
// of the two, not their sum; profiles/g2_decompress.md has the compiler's figures.  The budget is that of k_g2_subgroup_check: one wave per
// SIMD, one point per lane.  Integer VALU work throughout: no MFMA.
#include "engine.h"
#include "byte_stager.h"
#include "g2_decode.h"

#include <string>

namespace kzg {

template <bool WIRE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_g2_decompress(const uint4* __restrict__ bytes, uint4* __restrict__ out, uint32_t n, uint32_t first, uint32_t flags, uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t raw[16];
    g2_load_raw(raw, bytes + 4 * (size_t)i);
    G2Affine p;
    uint32_t kind = g2_decompress_point(p, raw);
    if (kind == G2_DECODE_OK && (flags & KZG_G2_CHECK_SUBGROUP) && !g2_in_subgroup(p)) kind = G2_BAD_SUBGROUP;
    if (kind == G2_DECODE_OK && (flags & KZG_G2_REJECT_GENERATOR) && g2_is_generator(p)) kind = G2_BAD_GENERATOR;
    uint32_t o[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) o[j] = 0;
    if (kind == G2_DECODE_OK) g2_point_to_words<WIRE>(o, p);
    else atomicMin(bad, (first + i) << 2 | kind);                   // first + i < 2^28
    g2_store_words(out + 8 * (size_t)i, o);
}

// -------------------------------------------------------------------------------------------------
// host driver (slot 0's workspace and stream, synchronised on return)
// -------------------------------------------------------------------------------------------------
// The bytes go up through a ByteStager (byte_stager.h: the pinned halves and their lifetime rules), and a kernel starts behind every
// G2_DECODE_LAUNCH points: a launch of one wave per SIMD fills the device with 65 536 lanes, and launches of one stream run one after
// the other.
constexpr size_t G2_DECODE_LAUNCH = 4 * STAGE_CHUNK_BYTES / 64;     // points per kernel launch

// n compressed points (host) -> d_points (device format, n x 128 B) when d_points != nullptr, else wire points to out_wire (host) through
// ws.bases.  *bad_word = index << 2 | kind of the smallest refused index, or 0xFFFFFFFF; out_wire is written only when no point is refused.
int32_t g2_decompress_run(kzg_ctx* ctx, const uint8_t* bytes, size_t n, uint32_t flags, uint4* d_points, uint64_t* out_wire, uint32_t* bad_word) {
    *bad_word = 0xFFFFFFFFu;
    if (n == 0) return KZG_OK;
    if (n > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    MsmWorkspace& ws = ctx->msm;
    hipStream_t st = ctx->stream;
    const bool wire = d_points == nullptr;
    KZG_HIP_TRY(ctx, ws.bases_wire.reserve(n * 64 + 16));
    if (wire) { KZG_HIP_TRY(ctx, ws.bases.reserve(n * 128)); d_points = ws.bases.as<uint4>(); }
    { const int32_t rc = msm_pinned_out(ctx, ws); if (rc != KZG_OK) return rc; }
    char* d_bytes = ws.bases_wire.as<char>();
    uint32_t* d_bad = reinterpret_cast<uint32_t*>(d_bytes + n * 64);
    ByteStager stager;
    hipError_t e = stager.init(st, ws.pinned_out);
    if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0xFF, 4, st);
    if (e == hipSuccess) {
        e = stager.push(bytes, n * 64, d_bytes, G2_DECODE_LAUNCH * 64, [&](size_t lo, size_t hi) {
            const size_t p0 = lo / 64;
            const uint32_t cnt = (uint32_t)((hi - lo) / 64);
            const dim3 grid((cnt + 255) / 256), block(256);
            const uint4* src = reinterpret_cast<const uint4*>(d_bytes + lo);
            if (wire) hipLaunchKernelGGL(k_g2_decompress<true>, grid, block, 0, st, src, d_points + 8 * p0, cnt, (uint32_t)p0, flags, d_bad);
            else hipLaunchKernelGGL(k_g2_decompress<false>, grid, block, 0, st, src, d_points + 8 * p0, cnt, (uint32_t)p0, flags, d_bad);
        });
    }
    uint32_t h_bad = 0xFFFFFFFFu;
    if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);                 // (on every path: byte_stager.h, and &h_bad is being written until here)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return set_error(ctx, e, "decoding compressed G2 points");
    *bad_word = h_bad;
    if (wire && h_bad == 0xFFFFFFFFu) {
        KZG_HIP_TRY(ctx, hipMemcpyAsync(out_wire, d_points, n * 128, hipMemcpyDeviceToHost, st));
        KZG_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return KZG_OK;
}

// the status of a bad word of g2_decompress_run (index << 2 | kind), its index to *bad_index, a line for kzg_ctx_last_error
int32_t g2_decode_status(kzg_ctx* ctx, const char* who, uint32_t bad_word, uint64_t* bad_index) {
    if (bad_word == 0xFFFFFFFFu) return KZG_OK;
    static const char* const what[4] = {"is not a compressed finite point below the modulus", "has no point on the twist", "is not in the order-r subgroup", "is the generator"};
    if (bad_index) *bad_index = bad_word >> 2;
    ctx->last_error = std::string(who) + ": point " + std::to_string(bad_word >> 2) + " " + what[bad_word & 3u];
    return (bad_word & 3u) == G2_BAD_DESERIALIZE ? KZG_ERR_DESERIALIZE : KZG_ERR_NOT_ON_CURVE;
}

}  // namespace kzg

KZG_BOUND_CHECK_EXPORTS(g2decode)
