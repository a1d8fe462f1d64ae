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
//   k_g2_locate_terms     the segmented form of k_g2_weighted (kzg_header_group_sums): the lanes lie in the sorted order of a key per
//                         point, [r]P per lane, then a segmented scan over the wave; the first lane of every (wave, segment) leaves a piece
//   k_g2_locate_fold      one wave per segment adds its pieces and leaves the segment's sum as a wire XYZZ value
// The tile and segment sums are normalised with one batched inversion on the host.  Everything here is integer VALU work: no MFMA.
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

// ---- segmented sums: one sum per SEGMENT of a sorted lane order (kzg_header_group_sums; the plan: host_locate.h) ------------------------------
// Segmented suffix scan over the wave, the shape of locate_seg_scan (multilocate.hip) on G2 values: afterwards a lane holds the sum of the
// values of lanes lane .. the last lane of its segment in this wave.  key = the lane's segment (0xFFFFFFFF: an idle lane, never joined).
// Every addition is the checked g2_add: equal operands, opposite operands and the identity all occur (duplicate headers under equal
// weights, a header beside its negation).
__device__ __forceinline__ void g2_seg_scan(G2Xyzz& c, uint32_t key, bool active, uint32_t lane) {
#pragma unroll 1
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t kd = __shfl_down(key, d, 64);
        const bool join = active && (lane + d < 64) && kd == key;
        if (!__any(join)) continue;                                  // wave-uniform: nobody has a partner at this distance
        G2Xyzz u;
        g2_shfl(u, c, d, true);
        if (!join) g2_set_inf(u);                                    // (the whole wave makes the call: adding the identity returns at once)
        g2_add_into(c, u);
    }
}

struct G2LocateArgs {
    const uint4* points;        // device affine format: point 2 i = C2_i, point 2 i + 1 = pi2_i
    uint32_t n_points, n_lanes;
    const uint32_t* perm;       // [sorted position] -> point
    const uint32_t* seg_of;     // [sorted position] -> segment
    const uint32_t* seg_off;    // n_seg + 1
    const uint32_t* part_off;   // n_seg + 1
    const uint4* weights;       // n_weights x 8 canonical u32 words; point p takes weight p >> 1
    uint32_t n_weights;
    int bits;
    int32_t* partial;           // XYZZ planes of G2, stride n_part
    uint32_t n_part;
};

// Lane t < n_lanes (sorted position): [w]P for P = points[perm[t]], w = weights[perm[t] >> 1]; an index out of range and an identity
// point give the identity, as an idle lane does.  Then the scan; the first lane of each (wave, segment) stores its piece at slot
// part_off[seg] + wave - seg_off[seg] / 64 (< part_off[seg + 1] = n_part at most, by host_locate.h's count of the waves a segment
// touches; the comparison with n_part keeps a store inside the buffer whatever the plan).  No lane returns before the scan.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_g2_locate_terms(G2LocateArgs a) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const bool active = t < a.n_lanes;
    G2Xyzz acc;
    g2_set_inf(acc);
    uint32_t key = 0xFFFFFFFFu;
    if (active) {
        const uint32_t idx = a.perm[t];
        key = a.seg_of[t];
        if (idx < a.n_points && (idx >> 1) < a.n_weights) {
            G2Affine p;
            if (g2_affine_load(p, a.points + 8 * (size_t)idx)) {
                const uint4 x = a.weights[2 * (size_t)(idx >> 1)], y = a.weights[2 * (size_t)(idx >> 1) + 1];
                const uint32_t k[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
                g2_mul_bits(acc, p, k, a.bits);
            }
        }
    }
    g2_seg_scan(acc, key, active, lane);
    const uint32_t kprev = __shfl_up(key, 1, 64);
    if (active && (lane == 0 || kprev != key)) {
        const uint32_t slot = a.part_off[key] + (t >> 6) - (a.seg_off[key] >> 6);
        if (slot < a.n_part) g2_store(a.partial, (size_t)a.n_part, slot, acc);
    }
}

// One wave per segment: workgroup j adds the partials [part_off[j], part_off[j + 1]), reduces by the shuffle tree of k_g2_weighted and
// leaves the 64 XYZZ wire words of the sum at out_wire[j].
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_g2_locate_fold(const int32_t* __restrict__ partial, uint32_t n_part, const uint32_t* __restrict__ part_off, uint32_t* __restrict__ out_wire) {
    const uint32_t j = blockIdx.x, lane = threadIdx.x;
    const uint32_t p0 = part_off[j], p1 = part_off[j + 1] < n_part ? part_off[j + 1] : n_part;
    G2Xyzz acc;
    g2_set_inf(acc);
#pragma unroll 1
    for (uint32_t p = p0 + lane; p < p1; p += 64) {
        G2Xyzz v;
        g2_load(v, partial, (size_t)n_part, p);
        g2_add_into(acc, v);
    }
#pragma unroll 1
    for (int d = 32; d >= 1; d >>= 1) {                             // every lane of the wave is here
        G2Xyzz u;
        g2_shfl(u, acc, d, true);
        g2_add_into(acc, u);
    }
    if (lane == 0) {
        uint32_t w[G2_WIRE_WORDS];
        g2_to_wire(w, acc);
        uint4* o = reinterpret_cast<uint4*>(out_wire + (size_t)j * G2_WIRE_WORDS);
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

// The plan is locate_plan (host_locate.h) over one key per POINT, plan.count = n_points lanes in sorted order; its arrays go to ctx->ml[1],
// the pieces to ctx->ml[2], the segment sums to ctx->ml[3].  out_seg_g2: plan.segs.size() affine wire points, one batched inversion.
int32_t g2_locate_segment_sums(kzg_ctx* ctx, const uint4* d_points, size_t n_points, const LocatePlan& plan, const uint32_t* weights_canonical, size_t n_weights,
                               int bits, uint64_t* out_seg_g2) {
    const size_t n_lanes = plan.count, S = plan.segs.size(), n_part = plan.part_off.back();
    if (n_lanes == 0) return KZG_OK;
    if (n_lanes != n_points || n_lanes > ((size_t)1 << 21) || n_weights == 0 || bits < 0 || bits > 256) return KZG_ERR_INVALID_ARG;
    RoctxRange range("kzg:g2_locate_segment_sums");
    int32_t rc = locate_upload_plan(ctx, plan);
    if (rc != KZG_OK) return rc;
    MsmWorkspace& ws = ctx->msm;
    KZG_HIP_TRY(ctx, ws.digits.reserve(n_weights * 32));
    KZG_HIP_TRY(ctx, ctx->ml[2].reserve(n_part * G2_LIMBS * 4));
    KZG_HIP_TRY(ctx, ctx->ml[3].reserve(S * G2_WIRE_WORDS * 4));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ws.digits.p, weights_canonical, n_weights * 32, hipMemcpyHostToDevice, ctx->stream));
    const uint32_t* d_plan = ctx->ml[1].as<uint32_t>();
    G2LocateArgs a;
    a.points = d_points; a.n_points = (uint32_t)n_points; a.n_lanes = (uint32_t)n_lanes;
    a.perm = d_plan; a.seg_of = d_plan + n_lanes; a.seg_off = d_plan + 2 * n_lanes; a.part_off = d_plan + 2 * n_lanes + S + 1;
    a.weights = ws.digits.as<uint4>(); a.n_weights = (uint32_t)n_weights; a.bits = bits;
    a.partial = ctx->ml[2].as<int32_t>(); a.n_part = (uint32_t)n_part;
    hipLaunchKernelGGL(k_g2_locate_terms, dim3((unsigned)((n_lanes + 255) / 256)), dim3(256), 0, ctx->stream, a);
    KZG_HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_g2_locate_fold, dim3((unsigned)S), dim3(64), 0, ctx->stream, a.partial, a.n_part, a.part_off, ctx->ml[3].as<uint32_t>());
    KZG_HIP_TRY(ctx, hipGetLastError());
    std::vector<uint32_t> wire(S * G2_WIRE_WORDS);
    KZG_HIP_TRY(ctx, hipMemcpyAsync(wire.data(), ctx->ml[3].p, wire.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    g2_tiles_to_affine(wire.data(), S, out_seg_g2);
    return KZG_OK;
}

}  // namespace kzg

KZG_BOUND_CHECK_EXPORTS(g2batch)
