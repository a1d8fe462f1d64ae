// fsdevice.hip — Fiat-Shamir hashing on the device, for transcripts that are MANY independent SHA-256 streams of one length (one stream is
// sequential and stays on the host: host_sha256.h).  The first consumer is the coset transcript of kzg_verify_multiproof_batch
// (host_fiat_shamir.h multiproof_r_powers_host): `count` item digests over 72 + 32 l bytes each, of values the call uploads anyway.
//
//   k_sha256_rows          one lane per message of row_len bytes (byte loads at any alignment): the primitive behind kzg_sha256_rows
//   k_coset_item_digests   one lane per item: the message is produced block by block from the wire values, the coset pair and the wire proof
//                          (coset_item_stream.h: Montgomery -> canonical, big-endian words, the compressed point), never stored; one flag
//                          word is set when an input is not canonical (the caller then derives the weights on the host)
//   k_coset_item_digests_bytes  the same digests from items in their serialized form (kzg_verify_multiproof_batch_bytes): the message is the value
//                          bytes as they are and the gnark-compressed proof reversed with its flag bits remapped; no field arithmetic, no flag
//   k_fr_powers_from_tables  out[i] = r^i as lo[i mod S] * hi[i div S] from two host-computed tables of about sqrt(count) wire scalars: wire
//                          form is the canonical representative, so the words equal those of the host's running product (powers_of)
// Shapes chosen: a workgroup is ONE wave (no LDS, no barrier); every lane of a wave is at the same block of its message, so the slot
// branches of coset_item_stream.h are wave-uniform.  A lane reads its values 32 bytes at a time at a stride of 32 l bytes, straight from
// global memory.  Not tried: staging tiles of values through LDS for large l, two items per lane for instruction-level parallelism, pinned
// staging of the digest copy.  Integer VALU work throughout: no MFMA.  Measured figures: profiles/fs_device.md.
#include "engine.h"
#include "coset_item_stream.h"
#include "host_fiat_shamir.h"
#include "host_coset_bytes.h"

#include <algorithm>
#include <vector>

namespace kzg {

constexpr uint32_t FS_LANES = 64;

__device__ __forceinline__ void fs_store_digest(uint4* __restrict__ out, size_t i, const uint32_t st[8]) {
    uint32_t o[8];
    sha256_digest_le_words(o, st);
    out[2 * i] = make_uint4(o[0], o[1], o[2], o[3]);
    out[2 * i + 1] = make_uint4(o[4], o[5], o[6], o[7]);
}

__global__ void __launch_bounds__(FS_LANES)
k_sha256_rows(const uint8_t* __restrict__ msgs, uint32_t row_len, uint32_t count, uint4* __restrict__ out) {
    const uint32_t i = blockIdx.x * FS_LANES + threadIdx.x;
    if (i >= count) return;
    const uint8_t* m = msgs + (size_t)i * row_len;
    const uint32_t nb = (uint32_t)sha256_n_blocks(row_len);
    uint32_t st[8], w[16];
    sha256_init_state(st);
#pragma unroll 1
    for (uint32_t b = 0; b < nb; ++b) {
        sha256_message_block(w, m, row_len, b);                       // (reads bytes below row_len only)
        sha256_compress(st, w);
    }
    fs_store_digest(out, i, st);
}

__global__ void __launch_bounds__(FS_LANES)
k_coset_item_digests(const uint4* __restrict__ ys, const uint64_t* __restrict__ cs, const uint64_t* __restrict__ ks, const uint4* __restrict__ proofs,
                     uint32_t count, uint32_t l, uint4* __restrict__ out, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * FS_LANES + threadIdx.x;
    if (i >= count) return;
    CosetItemSrc src;
    src.ys = reinterpret_cast<const uint32_t*>(ys + 2 * (size_t)i * l);
    src.proof = reinterpret_cast<const uint32_t*>(proofs + 4 * (size_t)i);
    src.c = cs[i];
    src.k = ks[i];
    src.l = l;
    const uint32_t nb = coset_item_blocks(l);
    uint32_t st[8], w[16], carry[2] = {0, 0}, bad = 0;
    sha256_init_state(st);
#pragma unroll 1
    for (uint32_t b = 0; b < nb; ++b) {
        coset_item_block(w, src, b, carry, bad);                      // (slots below l read value words, slot l the proof, later slots nothing)
        sha256_compress(st, w);
    }
    fs_store_digest(out, i, st);
    if (bad) atomicOr(flag, 1u);
}

// the same digests from serialized items: ys = l x 32 value bytes per item, proofs = 32 gnark-compressed bytes per item (coset_item_stream.h,
// the second producer)
__global__ void __launch_bounds__(FS_LANES)
k_coset_item_digests_bytes(const uint4* __restrict__ ys, const uint64_t* __restrict__ cs, const uint64_t* __restrict__ ks, const uint4* __restrict__ proofs,
                           uint32_t count, uint32_t l, uint4* __restrict__ out) {
    const uint32_t i = blockIdx.x * FS_LANES + threadIdx.x;
    if (i >= count) return;
    CosetItemBytesSrc src;
    src.ys = reinterpret_cast<const uint32_t*>(ys + 2 * (size_t)i * l);
    src.proof = reinterpret_cast<const uint32_t*>(proofs + 2 * (size_t)i);
    src.c = cs[i];
    src.k = ks[i];
    src.l = l;
    const uint32_t nb = coset_item_blocks(l);
    uint32_t st[8], w[16], carry[2] = {0, 0};
    sha256_init_state(st);
#pragma unroll 1
    for (uint32_t b = 0; b < nb; ++b) {
        coset_item_bytes_block(w, src, b, carry);
        sha256_compress(st, w);
    }
    fs_store_digest(out, i, st);
}

__global__ void __launch_bounds__(256)
k_fr_powers_from_tables(const uint4* __restrict__ lo, const uint4* __restrict__ hi, uint32_t log_s, uint32_t count, uint4* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t a = i & ((1u << log_s) - 1u), b = i >> log_s;
    const uint4 l0 = lo[2 * (size_t)a], l1 = lo[2 * (size_t)a + 1], h0 = hi[2 * (size_t)b], h1 = hi[2 * (size_t)b + 1];
    const uint32_t lw[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w}, hw[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
    Fr x, y;
    fe_unpack(x, lw);                                                 // r^a 2^256 as it is: < 2^256 < 5.3 m, normalised
    fe_from_wire(y, hw);                                              // r^(b S) 2^261 in (-m, 2m)
    fe_mul(x, x, y);                                                  // r^i 2^256: the wire residue, in (-m, 2m); |x y| < 10.6 m^2
    fe_canon(x);
    uint32_t o[8];
    fe_pack(o, x);
    out[2 * (size_t)i] = make_uint4(o[0], o[1], o[2], o[3]);
    out[2 * (size_t)i + 1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// -------------------------------------------------------------------------------------------------
// host drivers (ctx->stream, ctx->fs; called under ctx->mu, synchronised on return)
// -------------------------------------------------------------------------------------------------
// ctx->fs[1] of both device transcripts of `count` items: digests | lo | hi | flag, lo = S = 2^log_s entries of r^a and hi = H of r^(b S); S H >= count,
// both about sqrt(count)
struct FsBuffers { int log_s; size_t S, H; uint4 *d_digests, *d_lo, *d_hi; uint32_t* d_flag; };
static hipError_t fs_buffers(kzg_ctx* ctx, size_t count, FsBuffers* b) {
    const int bits = count <= 1 ? 0 : 64 - __builtin_clzll((unsigned long long)(count - 1)), log_s = (bits + 1) / 2;
    const size_t S = (size_t)1 << log_s, H = (count + S - 1) >> log_s;
    const hipError_t e = ctx->fs[1].reserve(count * 32 + (S + H) * 32 + 16);
    uint4* d = ctx->fs[1].as<uint4>();
    *b = FsBuffers{log_s, S, H, d, d + 2 * count, d + 2 * (count + S), reinterpret_cast<uint32_t*>(d + 2 * (count + S + H))};
    return e;
}
static int32_t fs_powers_from_transcript(kzg_ctx* ctx, const std::vector<uint8_t>& data, size_t count, const FsBuffers& b, uint4* d_weights, uint64_t* out_r_powers);

int32_t sha256_rows_run(kzg_ctx* ctx, const uint8_t* msgs, size_t row_len, size_t count, uint8_t* out_digests) {
    if (count == 0) return KZG_OK;
    hipStream_t st = ctx->stream;
    KZG_HIP_TRY(ctx, ctx->fs[0].reserve(std::max<size_t>(count * row_len, 16)));
    KZG_HIP_TRY(ctx, ctx->fs[1].reserve(count * 32));
    if (row_len) KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->fs[0].p, msgs, count * row_len, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_sha256_rows, dim3((unsigned)((count + FS_LANES - 1) / FS_LANES)), dim3(FS_LANES), 0, st, ctx->fs[0].as<uint8_t>(), (uint32_t)row_len,
                       (uint32_t)count, ctx->fs[1].as<uint4>());
    KZG_HIP_TRY(ctx, hipGetLastError());
    KZG_HIP_TRY(ctx, hipMemcpyAsync(out_digests, ctx->fs[1].p, count * 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return KZG_OK;
}

int32_t coset_r_powers_device(kzg_ctx* ctx, const uint64_t* commitments, size_t n_commitments, const uint64_t* commitment_indices, const uint4* d_ys,
                              const uint64_t* d_ks, const uint64_t* proofs, size_t count, size_t n, size_t l, uint4* d_weights, uint64_t* out_r_powers,
                              bool* fell_back) {
    using namespace kzg_host;
    RoctxRange range("kzg:multiproof_verify:r_powers (device)");
    *fell_back = false;
    if (count == 0) return KZG_OK;
    hipStream_t st = ctx->stream;
    FsBuffers b;
    KZG_HIP_TRY(ctx, fs_buffers(ctx, count, &b));
    KZG_HIP_TRY(ctx, ctx->fs[0].reserve(count * 72));                                      // proofs | commitment rows
    uint4* d_proofs = ctx->fs[0].as<uint4>();
    uint64_t* d_cs = reinterpret_cast<uint64_t*>(ctx->fs[0].as<uint8_t>() + count * 64);
    KZG_HIP_TRY(ctx, hipMemcpyAsync(d_proofs, proofs, count * 64, hipMemcpyHostToDevice, st));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(d_cs, commitment_indices, count * 8, hipMemcpyHostToDevice, st));
    KZG_HIP_TRY(ctx, hipMemsetAsync(b.d_flag, 0, 16, st));
    hipLaunchKernelGGL(k_coset_item_digests, dim3((unsigned)((count + FS_LANES - 1) / FS_LANES)), dim3(FS_LANES), 0, st, d_ys, d_cs, d_ks, d_proofs,
                       (uint32_t)count, (uint32_t)l, b.d_digests, b.d_flag);
    KZG_HIP_TRY(ctx, hipGetLastError());
    std::vector<uint8_t> data = coset_batch_transcript(commitments, n_commitments, count, n, l);       // (beside the kernel)
    uint32_t flag = 0;
    KZG_HIP_TRY(ctx, hipMemcpyAsync(data.data() + coset_batch_head(n_commitments), b.d_digests, count * 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(&flag, b.d_flag, 4, hipMemcpyDeviceToHost, st));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (flag) { *fell_back = true; return KZG_OK; }
    return fs_powers_from_transcript(ctx, data, count, b, d_weights, out_r_powers);
}

// the tail of both device transcripts: r from the complete batch transcript (host), its powers as one product of two table entries per lane
// into d_weights and to out_r_powers (host).  Synchronised on return
static int32_t fs_powers_from_transcript(kzg_ctx* ctx, const std::vector<uint8_t>& data, size_t count, const FsBuffers& b, uint4* d_weights, uint64_t* out_r_powers) {
    using namespace kzg_host;
    hipStream_t st = ctx->stream;
    const size_t S = b.S, H = b.H;
    uint64_t r[4];
    hash_to_r(data, r);                                                                   // the one sequential stream: 56 + 32 (M + count) bytes
    std::vector<uint64_t> tab(4 * (S + H));
    uint64_t* lo = tab.data();
    uint64_t* hi = lo + 4 * S;
    uint64_t step[4];
    fr_one(lo);
    for (size_t j = 1; j < S; ++j) fr_mul(lo + 4 * (j - 1), r, lo + 4 * j);
    fr_mul(lo + 4 * (S - 1), r, step);                                                    // r^S
    fr_one(hi);
    for (size_t j = 1; j < H; ++j) fr_mul(hi + 4 * (j - 1), step, hi + 4 * j);
    KZG_HIP_TRY(ctx, hipMemcpyAsync(b.d_lo, tab.data(), (S + H) * 32, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_fr_powers_from_tables, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, b.d_lo, b.d_hi, (uint32_t)b.log_s, (uint32_t)count, d_weights);
    KZG_HIP_TRY(ctx, hipGetLastError());
    KZG_HIP_TRY(ctx, hipMemcpyAsync(out_r_powers, d_weights, count * 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(st));                                           // (tab and out_r_powers are in use until here)
    return KZG_OK;
}

// The same weights from items ALREADY on the device in their serialized form (cosetbytes.hip: value bytes, gnark-compressed proofs): the second
// producer of coset_item_stream.h, no conversion and nothing to fall back from.  commitments_be and commitment_indices: host.  Synchronised on return
int32_t coset_r_powers_device_bytes(kzg_ctx* ctx, const uint8_t* commitments_be, size_t n_commitments, const uint64_t* commitment_indices, const uint4* d_ys_be,
                                    const uint64_t* d_ks, const uint4* d_proofs_be, size_t count, size_t n, size_t l, uint4* d_weights, uint64_t* out_r_powers) {
    using namespace kzg_host;
    RoctxRange range("kzg:multiproof_verify:r_powers (device, from bytes)");
    if (count == 0) return KZG_OK;
    hipStream_t st = ctx->stream;
    FsBuffers b;
    KZG_HIP_TRY(ctx, fs_buffers(ctx, count, &b));
    KZG_HIP_TRY(ctx, ctx->fs[0].reserve(count * 8 + 16));                                  // commitment rows
    uint64_t* d_cs = ctx->fs[0].as<uint64_t>();
    KZG_HIP_TRY(ctx, hipMemcpyAsync(d_cs, commitment_indices, count * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_coset_item_digests_bytes, dim3((unsigned)((count + FS_LANES - 1) / FS_LANES)), dim3(FS_LANES), 0, st, d_ys_be, d_cs, d_ks, d_proofs_be,
                       (uint32_t)count, (uint32_t)l, b.d_digests);
    KZG_HIP_TRY(ctx, hipGetLastError());
    std::vector<uint8_t> data = coset_batch_transcript_bytes(commitments_be, n_commitments, count, n, l);      // (beside the kernel)
    KZG_HIP_TRY(ctx, hipMemcpyAsync(data.data() + coset_batch_head(n_commitments), b.d_digests, count * 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return fs_powers_from_transcript(ctx, data, count, b, d_weights, out_r_powers);
}

}  // namespace kzg

KZG_BOUND_CHECK_EXPORTS(fsdevice)
