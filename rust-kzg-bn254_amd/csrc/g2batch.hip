// g2batch.hip — per-lane G2 chains for batches of untrusted points (g2_chain.h): the order-r subgroup test of every point and the
// weighted sums  sum_j [r_j]P_j  with SHORT weights chosen by the verifier (kzg_verify_length_proof_batch, kzg_g2_check_subgroup).
//
// Why not the bucket MSM of g2msm.hip: its fixed cost (sort, bucket reduction) is 13-18 ms per base set below 2^18 points
// (profiles/g2msm.md) and a header batch needs one sum per claimed length; 128-bit weights make plain double-and-add per lane the
// cheaper shape, and it is the shape of the subgroup test (a 63-bit chain per point) too.
//
//   k_g2_subgroup_check   one lane per point: [x + 1]P + psi([x]P) + psi^2([x]P) == psi^3([2x]P), atomicMin of the first failure
//   k_g2_weighted         one lane per (point, weight): [r]P, then the 64 lanes of a wave are summed by a shuffle tree; lane 0 leaves
//                         the tile's sum as a wire XYZZ value.  The host lays the lanes out so that a tile never spans two sums.
// The tile sums are normalised with one batched inversion on the host.  Everything here is integer VALU work: no MFMA.
//
// Register budget (profiles/header_batch.md has the compiler's figures): an XYZZ accumulator is 72 limb registers, the base point
// 36, a Karatsuba product in flight ~60 more, the subgroup test holds two accumulators: one wave per SIMD (the 512-entry file), one
// point per lane.
#include "engine.h"
#include "g2_chain.h"
#include "g2msm_plan.h"
#include "host_pairing.h"

#include <cstring>
#include <vector>

namespace kzg {

// *bad = the smallest index of a point that is neither the identity nor in the order-r subgroup (the caller sets it to 0xFFFFFFFF)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_g2_subgroup_check(const uint4* __restrict__ points, uint32_t n, uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G2Affine p;
    if (!g2_affine_load(p, points + 8 * (size_t)i)) return;         // the identity
    if (!g2_in_subgroup(p)) atomicMin(bad, i);
}

// Lane t: [w]P for P = points[lanes[t]] and w = weights[lanes[t] >> weight_shift]; an entry of 0xFFFFFFFF (padding of a tile), an index
// out of range and an identity point all give the identity.  Then a six-step shuffle tree per wave; out_wire[tile] = its sum.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_g2_weighted(const uint4* __restrict__ points, uint32_t n_points, const uint32_t* __restrict__ lanes, uint32_t n_lanes,
              const uint4* __restrict__ weights, uint32_t n_weights, uint32_t weight_shift, int bits, uint32_t* __restrict__ out_wire) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t idx = t < n_lanes ? lanes[t] : 0xFFFFFFFFu;
    G2Xyzz acc;
    g2_set_inf(acc);
    if (idx < n_points && (idx >> weight_shift) < n_weights) {
        G2Affine p;
        if (g2_affine_load(p, points + 8 * (size_t)idx)) {
            const uint4 a = weights[2 * (size_t)(idx >> weight_shift)], b = weights[2 * (size_t)(idx >> weight_shift) + 1];
            const uint32_t k[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            g2_mul_bits(acc, p, k, bits);
        }
    }
#pragma unroll 1
    for (int d = 32; d >= 1; d >>= 1) {                             // every lane of the wave is here: no lane returned above
        G2Xyzz u;
        g2_shfl(u, acc, d, true);
        g2_add_into(acc, u);
    }
    if ((threadIdx.x & 63) == 0 && t < n_lanes) {
        uint32_t w[G2_WIRE_WORDS];
        g2_to_wire(w, acc);
        uint4* o = reinterpret_cast<uint4*>(out_wire + (size_t)(t >> 6) * G2_WIRE_WORDS);
#pragma unroll
        for (int q = 0; q < (int)G2_WIRE_WORDS / 4; ++q) o[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    }
}

// -------------------------------------------------------------------------------------------------
// host driver (slot 0's workspace and stream, synchronised on return)
// -------------------------------------------------------------------------------------------------
namespace H = kzg_host;

int32_t g2_subgroup_check(kzg_ctx* ctx, const uint4* d_points, size_t n, int64_t* bad) {
    *bad = -1;
    if (n == 0) return KZG_OK;
    if (n > 0xFFFFFFF0u) return KZG_ERR_TOO_LARGE;
    MsmWorkspace& ws = ctx->msm;
    KZG_HIP_TRY(ctx, ws.count.reserve(16));
    uint32_t* d_bad = ws.count.as<uint32_t>();
    ws.count_zero_ptr = nullptr;                                    // (`count` no longer holds the zeros a table-mode sort left there)
    uint32_t h_bad = 0xFFFFFFFFu;
    KZG_HIP_TRY(ctx, hipMemcpyAsync(d_bad, &h_bad, 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_g2_subgroup_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_points, (uint32_t)n, d_bad);
    KZG_HIP_TRY(ctx, hipGetLastError());
    KZG_HIP_TRY(ctx, hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (h_bad != 0xFFFFFFFFu) *bad = (int64_t)h_bad;
    return KZG_OK;
}

// n wire XYZZ values (64 u32 each) -> affine wire points, one inversion for all of them (Montgomery's trick, as g2_horner does)
static void g2_tiles_to_affine(const uint32_t* wire, size_t n, uint64_t* out_g2) {
    std::vector<H::G2> pt(n);
    std::vector<H::Fq2> den(n), pre(n);
    H::Fq2 run = {H::FQ_ONE, H::fq_zero()};
    for (size_t w = 0; w < n; ++w) {
        H::Fq2 q[4];
        for (int k = 0; k < 4; ++k) { memcpy(q[k].c0.l, wire + w * G2_WIRE_WORDS + 16 * k, 32); memcpy(q[k].c1.l, wire + w * G2_WIRE_WORDS + 16 * k + 8, 32); }
        pt[w].inf = H::is_zero(q[2]);
        den[w] = pt[w].inf ? H::Fq2{H::FQ_ONE, H::fq_zero()} : H::mul(q[2], q[3]);       // ZZ ZZZ
        pre[w] = run;
        run = H::mul(run, den[w]);
        if (!pt[w].inf) { pt[w].x = H::mul(q[0], q[3]); pt[w].y = H::mul(q[1], q[2]); }    // X ZZZ, Y ZZ: over ZZ ZZZ they are X / ZZ, Y / ZZZ
    }
    H::Fq2 iv = H::inv(run);
    for (size_t w = n; w-- > 0;) {
        const H::Fq2 di = H::mul(iv, pre[w]);
        iv = H::mul(iv, den[w]);
        if (pt[w].inf) { memset(out_g2 + 16 * w, 0, 128); continue; }
        pt[w].x = H::mul(pt[w].x, di); pt[w].y = H::mul(pt[w].y, di);
        H::g2_to_wire(pt[w], out_g2 + 16 * w);
    }
}

int32_t g2_weighted_tile_sums(kzg_ctx* ctx, const uint4* d_points, size_t n_points, const uint32_t* lanes, size_t n_lanes, const uint32_t* weights_canonical,
                              size_t n_weights, uint32_t weight_shift, int bits, uint64_t* out_tiles_g2) {
    if (n_lanes == 0) return KZG_OK;
    if (n_lanes % 64 || n_lanes > 0xFFFFFF00u || n_points > 0xFFFFFFF0u || n_weights == 0 || bits < 0 || bits > 256) return KZG_ERR_INVALID_ARG;
    MsmWorkspace& ws = ctx->msm;
    const size_t tiles = n_lanes / 64;
    KZG_HIP_TRY(ctx, ws.sorted.reserve(n_lanes * 4));
    KZG_HIP_TRY(ctx, ws.digits.reserve(n_weights * 32));
    KZG_HIP_TRY(ctx, ws.out_wire.reserve(tiles * G2_WIRE_WORDS * 4));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ws.sorted.p, lanes, n_lanes * 4, hipMemcpyHostToDevice, ctx->stream));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ws.digits.p, weights_canonical, n_weights * 32, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_g2_weighted, dim3((unsigned)((n_lanes + 255) / 256)), dim3(256), 0, ctx->stream, d_points, (uint32_t)n_points, ws.sorted.as<uint32_t>(),
                       (uint32_t)n_lanes, ws.digits.as<uint4>(), (uint32_t)n_weights, weight_shift, bits, ws.out_wire.as<uint32_t>());
    KZG_HIP_TRY(ctx, hipGetLastError());
    std::vector<uint32_t> wire(tiles * G2_WIRE_WORDS);
    KZG_HIP_TRY(ctx, hipMemcpyAsync(wire.data(), ws.out_wire.p, wire.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    g2_tiles_to_affine(wire.data(), tiles, out_tiles_g2);
    return KZG_OK;
}

}  // namespace kzg

KZG_BOUND_CHECK_EXPORTS(g2batch)
