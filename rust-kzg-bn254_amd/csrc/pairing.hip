// pairing.hip — batches of pairing checks on the device: kzg_pairings_product_verify_batch, kzg_pairings_product_gt_batch, the host's
// kzg_pairings_product_gt, and kzg_ctx_set_locate_pairings (the located coset verifiers of capi_coset.hip send their leaves here).
//
// One check -- a product of its pairs' Miller functions, ONE final exponentiation, the is-one test -- is one lane's work (pairing_dev.h,
// fq12.h): the checks of a batch are independent, so a batch of n is n lanes, and nothing crosses lanes.
//
//   k_pairing_convert   one lane per pair: wire -> the device formats of curve.h / curve_g2.h, y^2 == x^3 + 3 and the twist equation,
//                       a flag byte per pair (1: G1 off the curve, 2: G2 off the twist)
//   k_pairing_checks    one lane per check, one wave per workgroup: pairing_check_dev; 96 wire words of GT and a verdict byte per check
//
// Where f lives: an Fq12 is 108 limbs and a check holds about ten of them beside the state of four pairs, so they are objects in private
// memory (scratch) and the Fq12 products are out-of-line loops around one inlined Fq2 product (fq12.h has the reasoning;
// profiles/pairing_device.md the compiler's figures).  A check costs the same ~40 000 Fq products whatever the batch: the kernel's time
// is that of ONE check until every SIMD has a wave (64 checks per wave), which is what the batch form is for.
#include "engine.h"
#include "host_pairing_batch.h"

#include <cstring>
#include <vector>

namespace kzg {

__global__ void __launch_bounds__(256)
k_pairing_convert(const uint4* __restrict__ g1_wire, const uint4* __restrict__ g2_wire, uint32_t n, uint4* __restrict__ g1_dev, uint4* __restrict__ g2_dev,
                  uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t a[16], b[32], oa[16], ob[32];
#pragma unroll
    for (int q = 0; q < 4; ++q) { const uint4 v = g1_wire[4 * (size_t)i + q]; a[4 * q] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w; }
#pragma unroll
    for (int q = 0; q < 8; ++q) { const uint4 v = g2_wire[8 * (size_t)i + q]; b[4 * q] = v.x; b[4 * q + 1] = v.y; b[4 * q + 2] = v.z; b[4 * q + 3] = v.w; }
    flags[i] = (uint8_t)pairing_pair_to_device(oa, ob, a, b);
#pragma unroll
    for (int q = 0; q < 4; ++q) g1_dev[4 * (size_t)i + q] = make_uint4(oa[4 * q], oa[4 * q + 1], oa[4 * q + 2], oa[4 * q + 3]);
#pragma unroll
    for (int q = 0; q < 8; ++q) g2_dev[8 * (size_t)i + q] = make_uint4(ob[4 * q], ob[4 * q + 1], ob[4 * q + 2], ob[4 * q + 3]);
}

// Check c covers the pairs [offsets[c], offsets[c + 1]) (the host has checked that the offsets rise and end at the number of pairs
// converted).  out_gt may be null.
__global__ void __launch_bounds__(64)
k_pairing_checks(const uint32_t* __restrict__ g1_dev, const uint32_t* __restrict__ g2_dev, const uint32_t* __restrict__ offsets, uint32_t n_checks,
                 const PairingConsts* __restrict__ consts, uint32_t* __restrict__ out_gt, uint8_t* __restrict__ out_ok) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_checks) return;
    uint32_t gt[96];
    const bool ok = pairing_check_dev(gt, g1_dev, g2_dev, offsets[c], offsets[c + 1], *consts);
    out_ok[c] = ok ? 1 : 0;
    if (out_gt) {
#pragma unroll 1
        for (int j = 0; j < 96; ++j) out_gt[96 * (size_t)c + j] = gt[j];
    }
}

// -------------------------------------------------------------------------------------------------
// host driver
// -------------------------------------------------------------------------------------------------
namespace H = kzg_host;
static_assert(PAIRING_RUN_MAX_PAIRS == H::PAIRING_BATCH_MAX_PAIRS, "engine.h states the limit of host_pairing_batch.h");

// the constants of the device pairing in ctx->pr[3], uploaded at the context's first batch (under ctx->mu, as every buffer of a context)
static int32_t pairing_consts_device(kzg_ctx* ctx, const PairingConsts** out) {
    if (!ctx->pr_consts_ready) {
        static const struct Built { PairingConsts c; bool ok; Built() { ok = H::pairing_consts_build(&c); } } built;     // once per process
        if (!built.ok) { ctx->last_error = "pairing constants: a table of host_pairing.h has an unexpected shape"; return KZG_ERR_DEVICE; }
        KZG_HIP_TRY(ctx, ctx->pr[3].reserve(sizeof(PairingConsts)));
        KZG_HIP_TRY(ctx, hipMemcpyAsync(ctx->pr[3].p, &built.c, sizeof(PairingConsts), hipMemcpyHostToDevice, ctx->stream));
        KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->pr_consts_ready = true;
    }
    *out = ctx->pr[3].as<PairingConsts>();
    return KZG_OK;
}

// The checks of one call.  The caller holds ctx->mu, has set the device and has passed pairing_batch_check_args.  Both outputs are host
// arrays and either may be null; nothing is written unless KZG_OK is returned.  Synchronised on return.
int32_t pairing_batch_run(kzg_ctx* ctx, const uint64_t* g1s_xy, const uint64_t* g2s, const uint64_t* pair_offsets, size_t n_checks, size_t total, uint8_t* out_ok,
                          uint64_t* out_gt, uint64_t* bad_index) {
    if (n_checks == 0) return KZG_OK;
    RoctxRange range("kzg:pairing_batch");
    const H::PairingBatchPlan p = H::pairing_batch_plan(n_checks, total);
    const PairingConsts* d_consts = nullptr;
    { const int32_t rc = pairing_consts_device(ctx, &d_consts); if (rc != KZG_OK) return rc; }
    KZG_HIP_TRY(ctx, ctx->pr[0].reserve(p.wire_bytes + 256));
    KZG_HIP_TRY(ctx, ctx->pr[1].reserve(p.dev_bytes + 256));
    KZG_HIP_TRY(ctx, ctx->pr[2].reserve(p.out_bytes + 256));
    uint8_t *w = ctx->pr[0].as<uint8_t>(), *d = ctx->pr[1].as<uint8_t>(), *o = ctx->pr[2].as<uint8_t>();
    std::vector<uint32_t> off32(n_checks + 1);
    for (size_t i = 0; i <= n_checks; ++i) off32[i] = (uint32_t)pair_offsets[i];
    KZG_HIP_TRY(ctx, hipMemcpyAsync(d + p.dev_offsets, off32.data(), off32.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    std::vector<uint8_t> flags(total);
    if (total) {
        KZG_HIP_TRY(ctx, hipMemcpyAsync(w + p.wire_g1, g1s_xy, total * 64, hipMemcpyHostToDevice, ctx->stream));
        KZG_HIP_TRY(ctx, hipMemcpyAsync(w + p.wire_g2, g2s, total * 128, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_pairing_convert, dim3(p.convert_blocks), dim3(256), 0, ctx->stream, reinterpret_cast<const uint4*>(w + p.wire_g1),
                           reinterpret_cast<const uint4*>(w + p.wire_g2), (uint32_t)total, reinterpret_cast<uint4*>(d + p.dev_g1), reinterpret_cast<uint4*>(d + p.dev_g2),
                           d + p.dev_flags);
        KZG_HIP_TRY(ctx, hipGetLastError());
        KZG_HIP_TRY(ctx, hipMemcpyAsync(flags.data(), d + p.dev_flags, total, hipMemcpyDeviceToHost, ctx->stream));
        KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        // the host entry's order: every G1 input first, then the G2 inputs
        for (uint32_t bit : {1u, 2u})
            for (size_t k = 0; k < total; ++k)
                if (flags[k] & bit) {
                    if (bad_index) *bad_index = (uint64_t)k;
                    ctx->last_error = "pairing batch: the " + std::string(bit == 1 ? "G1" : "G2") + " point of pair " + std::to_string(k) + " is not on its curve";
                    return bit == 1 ? KZG_ERR_G1_NOT_ON_CURVE : KZG_ERR_G2_TAU_NOT_ON_CURVE;
                }
    }
    hipLaunchKernelGGL(k_pairing_checks, dim3(p.check_blocks), dim3(H::PAIRING_BLOCK), 0, ctx->stream, reinterpret_cast<const uint32_t*>(d + p.dev_g1),
                       reinterpret_cast<const uint32_t*>(d + p.dev_g2), reinterpret_cast<const uint32_t*>(d + p.dev_offsets), (uint32_t)n_checks, d_consts,
                       out_gt ? reinterpret_cast<uint32_t*>(o + p.out_gt) : nullptr, o + p.out_ok);
    KZG_HIP_TRY(ctx, hipGetLastError());
    std::vector<uint8_t> ok(n_checks);
    std::vector<uint64_t> gt(out_gt ? n_checks * 48 : 0);
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ok.data(), o + p.out_ok, n_checks, hipMemcpyDeviceToHost, ctx->stream));
    if (out_gt) KZG_HIP_TRY(ctx, hipMemcpyAsync(gt.data(), o + p.out_gt, n_checks * 384, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (out_ok) memcpy(out_ok, ok.data(), n_checks);
    if (out_gt) memcpy(out_gt, gt.data(), n_checks * 384);
    return KZG_OK;
}

}  // namespace kzg

using namespace kzg;

static int32_t pairing_batch_entry(kzg_ctx* ctx, const uint64_t* g1s_xy, const uint64_t* g2s, const uint64_t* pair_offsets, size_t n_checks, uint8_t* out_ok,
                                   uint64_t* out_gt, const void* required_out, uint64_t* bad_index) {
    size_t total = 0;
    { const int32_t rc = kzg_host::pairing_batch_check_args(ctx, g1s_xy, g2s, pair_offsets, n_checks, required_out, &total); if (rc != KZG_OK) return rc; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return pairing_batch_run(ctx, g1s_xy, g2s, pair_offsets, n_checks, total, out_ok, out_gt, bad_index);
}

int32_t kzg_pairings_product_verify_batch(kzg_ctx* ctx, const uint64_t* g1s_xy, const uint64_t* g2s, const uint64_t* pair_offsets, size_t n_checks, uint8_t* out_ok,
                                          uint64_t* bad_index) {
    return pairing_batch_entry(ctx, g1s_xy, g2s, pair_offsets, n_checks, out_ok, nullptr, out_ok, bad_index);
}

int32_t kzg_pairings_product_gt_batch(kzg_ctx* ctx, const uint64_t* g1s_xy, const uint64_t* g2s, const uint64_t* pair_offsets, size_t n_checks, uint64_t* out_gt_mont,
                                      uint64_t* bad_index) {
    return pairing_batch_entry(ctx, g1s_xy, g2s, pair_offsets, n_checks, nullptr, out_gt_mont, out_gt_mont, bad_index);
}

int32_t kzg_pairings_product_gt(const uint64_t* g1s_xy, const uint64_t* g2s, size_t count, uint64_t* out_gt_mont) {
    if (!out_gt_mont || (count && (!g1s_xy || !g2s)) || count > ((size_t)1 << 30)) return KZG_ERR_INVALID_ARG;
    using namespace kzg_host;
    std::vector<G1> ps(count);
    std::vector<G2> qs(count);
    for (size_t k = 0; k < count; ++k) { ps[k] = g1_from_wire(g1s_xy + 8 * k); if (!g1_on_curve(ps[k])) return KZG_ERR_G1_NOT_ON_CURVE; }
    for (size_t k = 0; k < count; ++k) { qs[k] = g2_from_wire(g2s + 16 * k); if (!g2_on_curve(qs[k])) return KZG_ERR_G2_TAU_NOT_ON_CURVE; }
    kzg_host::Fq12 gt;
    (void)pairings_product_gt(ps.data(), qs.data(), (int)count, &gt, host_parallel_for);       // degenerate: all zero
    memcpy(out_gt_mont, gt.c, 384);
    return KZG_OK;
}

int32_t kzg_ctx_set_locate_pairings(kzg_ctx* ctx, int32_t mode) {
    if (!ctx || (mode != 0 && mode != 1)) return KZG_ERR_INVALID_ARG;
    ctx->locate_pairings.store(mode);
    return KZG_OK;
}

KZG_BOUND_CHECK_EXPORTS(pairing)
