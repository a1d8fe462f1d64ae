// multilocate.hip — the device side of locating the bad items of a rejected batch of coset proofs (capi_coset.hip kzg_coset_group_sums,
// kzg_verify_multiproof_batch_locate; the plan: host_locate.h).  The batch equation of multiverify.hip is linear in the set of items, so
// for ANY partition of the N items into groups the device can produce, in one pass, the two G1 sums of every group's own equation:
//
//     L_g     = sum_{i in g} r_i pi_i
//     A_{g,t} = sum_{i in g} r_i w^(-k_i t) IFFT_l(ys_i)_t                                      (this file, then n_groups MSMs over srs[0 .. l))
//     R_g     = sum_{i in g} (r_i C_{c_i} + r_i w^(k_i l) pi_i)  -  sum_t A_{g,t} [tau^t]_1     (the first sum: this file)
//
// and the host searches a tree of those sums with one pairing check per step.  The items are sorted by group on the host as a
// PERMUTATION (stable counting sort) with segment offsets; the values stay where the caller's order put them and every kernel below reads
// through the permutation.  Only non-empty groups ("segments") reach the device.
//
// Shapes chosen (the plain ones; profiles/multiproof_locate.md has the figures):
//   * coefficients: k_coset_interp<.., SEG = true> (coset_kernels.h: the tile transform of the batch kernel) writes the weighted, twisted
//     row of every ITEM back over its values as canonical wire words; k_coset_seg_sum then adds the rows of each segment, cb = min(l, 256)
//     columns and 256 / cb row groups per workgroup, folded by the LDS tree of the batch kernel.  l > 1024: ntt_run per coset as in
//     multiverify.hip, k_coset_twist_rows in place, the same segmented sum.  Not fused: no measurement asked for it.
//   * point sums: k_locate_terms, one lane per SORTED item: [r_i] pi_i and [r_i] C_{c_i} + [r_i w^(k_i l)] pi_i with the GLV
//     multiplication of glv.h (three of them), then a segmented suffix scan over wave shuffles (the scan of k_msm_accumulate: a lane joins
//     the lane d above it while both are in one segment), so that the first lane of every (wave, segment) holds that piece's sum and
//     stores it at a slot the host planned.  k_locate_fold, one wave per (segment, sum), adds a segment's partials and leaves XYZZ wire
//     words; the host subtracts the MSM results and normalises.
//   * every exceptional case of the XYZZ law is explicit in curve.h xyzz_add (identity operands, P + P, P + (-P)) and in
//     xyzz_scalar_mul (identity base, zero scalar).  Points are validated on upload (points_wire_to_device with the curve check).
//   * no atomics, no floating point; the sums are group elements and leave as canonical affine words, so equal inputs give equal bits
//     whatever the order of the items inside a group and whatever the grid.
//   * the header batch (capi_g2.hip kzg_header_group_sums) takes the same two kernels with ONE sum per segment, U_g = sum_{i in g} r_i C_i:
//     the template parameter SUMS of k_locate_terms / k_locate_fold, driven by locate_group_sums_g1_device.
// Not tried: a joint (Shamir) chain for the two multiplications of pi_i, lane pairs (glv_lanes.h), a fused interpolation + segment sum.
#include "coset_kernels.h"
#include "glv.h"
#include "host_locate.h"

#include <algorithm>

namespace kzg {

// l > 1024: rows = count x l canonical wire values IFFT_l(ys_i) (ntt_run, 1 / l included) -> rows[i][t] *= r_i w^(-k_i t), in place
__global__ void __launch_bounds__(256)
k_coset_twist_rows(uint4* __restrict__ rows, const uint64_t* __restrict__ ks, const uint4* __restrict__ weights, uint32_t count, int log_l, int log_n, MvTables tb) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ((size_t)count << log_l)) return;
    const uint32_t i = (uint32_t)(e >> log_l), t = (uint32_t)e & ((1u << log_l) - 1u);
    const uint64_t n_mask = ((uint64_t)1 << log_n) - 1;
    Fr v, s, kin;
#pragma unroll
    for (int j = 0; j < NL; ++j) kin.l[j] = (int32_t)FrParams::K_IN[j];
    mv_load_words(v, rows + 2 * e);                                  // < 2^256 < 5.3 m
    mv_load_words(s, weights + 2 * (size_t)i);
    fe_mul(s, s, kin);                                               // wire -> internal: (-m, 2m)
    const uint32_t ex = (uint32_t)((ks[i] * (uint64_t)t) & n_mask);
    if (ex != 0) {
        Fr w;
        mv_root_pow(w, tb, ex);
        fe_mul(s, s, w);
    }
    fe_mul(v, v, s);                                                 // |v s| < 5.3 m * 2 m; the product is normalised, in (-m, 2m)
    mv_store_canonical(rows + 2 * e, v);
}

// out[j][t] = sum over the sorted positions s of segment j of rows[perm[s]][t], canonical wire words.  Workgroup j (l >> log_cb) + b takes
// the cb = min(l, 256) columns from b cb on with 256 / cb row groups, folded by the tree of k_coset_interp.  The rows are canonical
// words (k_coset_interp<.., true>, k_coset_twist_rows): in [0, m), inside mv_lazy_add's (-m, 2m).
__global__ void __launch_bounds__(256)
k_coset_seg_sum(const uint4* __restrict__ rows, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ seg_off, int log_l, int log_cb, uint4* __restrict__ out) {
    __shared__ int32_t x[NL * 256];
    const uint32_t tid = threadIdx.x, cb = 1u << log_cb, per_seg = 1u << (log_l - log_cb);
    const uint32_t seg = blockIdx.x >> (log_l - log_cb), col = (blockIdx.x & (per_seg - 1)) * cb + (tid & (cb - 1));
    const uint32_t rg = tid >> log_cb, groups = 256u >> log_cb;
    const uint32_t s0 = seg_off[seg], s1 = seg_off[seg + 1];
    Fr acc;
    fe_set_zero(acc);
    uint32_t pending = 0;
#pragma unroll 1
    for (uint32_t s = s0 + rg; s < s1; s += groups) {
        Fr v;
        mv_load_words(v, rows + 2 * (((size_t)perm[s] << log_l) + col));
        const bool reduce = ++pending == 32;
        if (reduce) pending = 0;
        mv_lazy_add(acc, v, reduce);                                 // |acc| < 2 m + 32 * 2 m = 66 m between two reductions
    }
    fe_reduce(acc);                                                  // |acc| < 66 m -> (-m, 2m), normalised
    mv_planes_store(x, 256, tid, acc);
    __syncthreads();
    mv_fold(x, 256, cb, tid);
    if (tid < cb) {
        Fr v;
        mv_planes_load(v, x, 256, tid);                              // (-0.0001 m, 1.0001 m) after a fold, (-m, 2m) without one
        mv_store_canonical(out + 2 * (((size_t)seg << log_l) + col), v);
    }
}

// Out of line: three multiplications per lane inlined are three copies of the 127-step chain
__device__ __noinline__ void locate_term(Xyzz& r, const uint4* __restrict__ scalar, const uint4* __restrict__ point) { glv_term(r, scalar, point); }

// Segmented suffix scan over the wave: afterwards lane = the sum of the values of lanes lane .. the last lane of its segment in this
// wave.  key = the lane's segment (0xFFFFFFFF: an idle lane, never joined).  After the step of distance d a lane holds the sum of the
// next 2 d lanes of its segment: lane + d is in the segment only if every lane between is (segments are runs of sorted positions).
__device__ __forceinline__ void locate_seg_scan(Xyzz& c, uint32_t key, bool active, uint32_t lane) {
#pragma unroll 1
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t kd = __shfl_down(key, d, 64);
        const bool join = active && (lane + d < 64) && kd == key;
        if (!__any(join)) continue;                                  // wave-uniform: nobody has a partner at this distance
        Xyzz u;
        xyzz_shfl_down(u, c, d);
        if (join) {
            Xyzz r;
            xyzz_add<true>(r, c, u);
            c = r;
        }
    }
}

struct LocateArgs {
    const uint4* points;        // device affine format: n_proofs proofs, then the commitments
    uint32_t n_proofs, count;
    const uint32_t* perm;       // [sorted position] -> item
    const uint32_t* seg_of;     // [sorted position] -> segment
    const uint32_t* seg_off;    // n_seg + 1
    const uint32_t* part_off;   // n_seg + 1
    const uint64_t* ci;         // [item] -> commitment row (< the number of commitments, checked by the host)
    const uint4* w;             // [item] r_i (wire)
    const uint4* w2;            // [item] r_i w^(k_i l) (wire)
    int32_t* partial;           // XYZZ planes, stride 2 n_part: the L pieces at [0, n_part), the R pieces at [n_part, 2 n_part)
    uint32_t n_part;
};

// Lane s < count (sorted position): item i = perm[s]; a = [r_i] pi_i, b = [r_i] C_{c_i} + [r_i w^(k_i l)] pi_i; then the scan; the first
// lane of each (wave, segment) stores both sums at slot part_off[seg] + wave - seg_off[seg] / 64 (< part_off[seg + 1] by host_locate.h's
// count of the waves a segment touches).  No lane returns before the scan.
// SUMS = 1 (the header batch, capi_g2.hip): the one sum [w_i] points[i] per segment, no second scalar, no commitment row.
template <int SUMS>
__global__ void __launch_bounds__(256)
k_locate_terms(LocateArgs a) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const bool active = s < a.count;
    Xyzz l, r;
    xyzz_set_inf(l);
    if (SUMS == 2) xyzz_set_inf(r);
    uint32_t key = 0xFFFFFFFFu;
    if (active) {
        const uint32_t i = a.perm[s];
        key = a.seg_of[s];
        const uint4* proof = a.points + 4 * (size_t)i;
        locate_term(l, a.w + 2 * (size_t)i, proof);
        if (SUMS == 2) {
            Xyzz t, u;
            locate_term(t, a.w2 + 2 * (size_t)i, proof);
            locate_term(u, a.w + 2 * (size_t)i, a.points + 4 * ((size_t)a.n_proofs + (size_t)a.ci[i]));
            xyzz_add<true>(r, u, t);
        }
    }
    locate_seg_scan(l, key, active, lane);
    if (SUMS == 2) locate_seg_scan(r, key, active, lane);
    const uint32_t kprev = __shfl_up(key, 1, 64);
    if (active && (lane == 0 || kprev != key)) {
        const uint32_t slot = a.part_off[key] + (s >> 6) - (a.seg_off[key] >> 6);
        xyzz_store(a.partial, SUMS * (size_t)a.n_part, slot, l);
        if (SUMS == 2) xyzz_store(a.partial, 2 * (size_t)a.n_part, (size_t)a.n_part + slot, r);
    }
}

// One wave per (segment, sum): workgroup SUMS j + q adds the partials [part_off[j], part_off[j + 1]) of sum q (0: L, 1: R) and leaves the 32
// XYZZ wire words at out[SUMS j + q].
template <int SUMS>
__global__ void __launch_bounds__(64)
k_locate_fold(const int32_t* __restrict__ partial, uint32_t n_part, const uint32_t* __restrict__ part_off, uint32_t* __restrict__ out_wire) {
    const uint32_t j = blockIdx.x / SUMS, q = blockIdx.x % SUMS, lane = threadIdx.x;
    const uint32_t p0 = part_off[j], p1 = part_off[j + 1];
    Xyzz acc;
    xyzz_set_inf(acc);
#pragma unroll 1
    for (uint32_t p = p0 + lane; p < p1; p += 64) {
        Xyzz v, t;
        xyzz_load(v, partial, SUMS * (size_t)n_part, (size_t)q * n_part + p);
        xyzz_add<true>(t, acc, v);
        acc = t;
    }
#pragma unroll 1
    for (int d = 32; d >= 1; d >>= 1) {                              // every lane of the wave is here
        Xyzz u;
        xyzz_shfl_down(u, acc, d);
        if ((int)lane < d) {
            Xyzz t;
            xyzz_add<true>(t, acc, u);
            acc = t;
        }
    }
    if (lane == 0) {
        uint32_t w[32];
        xyzz_to_wire(w, acc);
        uint4* o = reinterpret_cast<uint4*>(out_wire + (size_t)blockIdx.x * 32);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    }
}

// ---- host drivers: enqueued on ctx->stream, called under ctx->mu with the arguments checked (capi_coset.hip) -----------------------------

// The plan's arrays -> ctx->ml[1]: perm | seg_of | seg_off | part_off (uint32 each)
int32_t locate_upload_plan(kzg_ctx* ctx, const LocatePlan& plan) {
    const size_t N = plan.count, S = plan.segs.size();
    KZG_HIP_TRY(ctx, ctx->ml[1].reserve((2 * N + 2 * (S + 1)) * 4 + 64));
    uint32_t* d = ctx->ml[1].as<uint32_t>();
    KZG_HIP_TRY(ctx, hipMemcpyAsync(d, plan.perm.data(), N * 4, hipMemcpyHostToDevice, ctx->stream));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(d + N, plan.seg_of.data(), N * 4, hipMemcpyHostToDevice, ctx->stream));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(d + 2 * N, plan.seg_off.data(), (S + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(d + 2 * N + S + 1, plan.part_off.data(), (S + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    return KZG_OK;
}

// d_ys count x l wire values (OVERWRITTEN by the items' rows), d_ks, d_weights as for coset_interpolate_rlc_device; the plan uploaded by
// locate_upload_plan -> ctx->ml[0]: segs x l canonical wire coefficients A_{g,t}, segment-major.  count > 0.
int32_t coset_group_coeffs_device(kzg_ctx* ctx, uint4* d_ys, const uint64_t* d_ks, const uint4* d_weights, const LocatePlan& plan, size_t n, size_t l) {
    RoctxRange range("kzg:coset_group_coeffs");
    const int32_t rc = coset_item_rows_device(ctx, d_ys, d_ks, d_weights, plan.count, n, l, false);
    return rc != KZG_OK ? rc : coset_seg_sums_device(ctx, d_ys, plan, l);
}

// The first half: row i of d_ys, the l wire values of item i, becomes r_i w^(-k_i t) IFFT_l(ys_i)_t, canonical wire words.  The rows depend on
// the items alone, not on how a plan groups them.  transformed (l > 1024 only): d_ys already holds IFFT_l(ys_i), 1 / l included -- what the
// ntt_run per coset of coset_interpolate_rlc_device leaves when the batch equation has run over the same buffer; the loop below makes the same
// calls, so only the twist is left to do.  count > 0.
int32_t coset_item_rows_device(kzg_ctx* ctx, uint4* d_ys, const uint64_t* d_ks, const uint4* d_weights, size_t count, size_t n, size_t l, bool transformed) {
    hipStream_t st = ctx->stream;
    const int log_n = __builtin_ctzll(n), log_l = __builtin_ctzll(l);
    NttTables nt;
    int32_t rc = ntt_get_tables(ctx, log_n, true, &nt);
    if (rc != KZG_OK) return rc;
    MvTables tb{nt.lo, nt.hi, nt.lo_len, nt.hi_len, nt.lo_bits};
    if (l > MV_LDS_MAX_L) {
        for (size_t i = 0; i < count && !transformed; ++i) {
            rc = ntt_run(ctx, d_ys + 2 * i * l, l, true, st, &ctx->mv_ntt);
            if (rc != KZG_OK) return rc;
        }
        hipLaunchKernelGGL(k_coset_twist_rows, dim3((unsigned)((count * l + 255) / 256)), dim3(256), 0, st, d_ys, d_ks, d_weights, (uint32_t)count, log_l, log_n, tb);
    } else {
        const uint32_t E = l == 1024 ? 1024u : 512u, cpt = E >> log_l;
        const uint32_t tiles = (uint32_t)((count + cpt - 1) / cpt), groups = std::min(tiles, MV_MAX_GROUPS);
        MvArgs a;
        a.ys = d_ys; a.ks = d_ks; a.weights = d_weights; a.count = (uint32_t)count; a.log_l = log_l; a.log_n = log_n; a.tiles = tiles; a.tb = tb;
        a.partial = nullptr;
        a.rows = d_ys;
        const size_t lds = mv_interp_lds_bytes(E, l);
        if (E == 1024) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_coset_interp<4, true>), dim3(groups), dim3(256), lds, st, a);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_coset_interp<2, true>), dim3(groups), dim3(256), lds, st, a);
    }
    KZG_HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

// The second half: the rows of each segment of the plan (uploaded by locate_upload_plan; perm may name a subset of the items) added up ->
// ctx->ml[0]: segs x l canonical wire coefficients, segment-major.  plan.segs is not empty.
int32_t coset_seg_sums_device(kzg_ctx* ctx, const uint4* d_rows, const LocatePlan& plan, size_t l) {
    const size_t S = plan.segs.size();
    const int log_l = __builtin_ctzll(l);
    KZG_HIP_TRY(ctx, ctx->ml[0].reserve(S * l * 32));
    const uint32_t* d_plan = ctx->ml[1].as<uint32_t>();
    const int log_cb = std::min(log_l, 8);
    hipLaunchKernelGGL(k_coset_seg_sum, dim3((unsigned)(S << (log_l - log_cb))), dim3(256), 0, ctx->stream, d_rows, d_plan, d_plan + 2 * plan.count, log_l, log_cb, ctx->ml[0].as<uint4>());
    KZG_HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

// d_points: count proofs then the commitments (device format); d_ci / d_w / d_w2 per item (caller order); the plan uploaded by
// locate_upload_plan -> out_xyzz: per segment the XYZZ wire words (16 u64 each) of sum r_i pi_i and of sum (r_i C_{c_i} + r_i w^(k_i l) pi_i).
// Synchronised on return.  count > 0.  n_proofs: where the commitments begin in d_points (0: at plan.count; a plan over a subset of the items
// has fewer lanes than there are proofs).
int32_t locate_point_sums_device(kzg_ctx* ctx, const uint4* d_points, const uint64_t* d_ci, const uint4* d_w, const uint4* d_w2, const LocatePlan& plan, uint64_t* out_xyzz,
                                 size_t n_proofs) {
    RoctxRange range("kzg:locate_point_sums");
    const size_t N = plan.count, S = plan.segs.size(), n_part = plan.part_off.back();
    KZG_HIP_TRY(ctx, ctx->ml[2].reserve(2 * n_part * 4 * NL * 4));
    KZG_HIP_TRY(ctx, ctx->ml[3].reserve(S * 2 * 128));
    const uint32_t* d_plan = ctx->ml[1].as<uint32_t>();
    LocateArgs a;
    a.points = d_points; a.n_proofs = (uint32_t)(n_proofs ? n_proofs : N); a.count = (uint32_t)N;
    a.perm = d_plan; a.seg_of = d_plan + N; a.seg_off = d_plan + 2 * N; a.part_off = d_plan + 2 * N + S + 1;
    a.ci = d_ci; a.w = d_w; a.w2 = d_w2;
    a.partial = ctx->ml[2].as<int32_t>(); a.n_part = (uint32_t)n_part;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_locate_terms<2>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, a);
    KZG_HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_locate_fold<2>), dim3((unsigned)(2 * S)), dim3(64), 0, ctx->stream, a.partial, a.n_part, a.part_off, ctx->ml[3].as<uint32_t>());
    KZG_HIP_TRY(ctx, hipGetLastError());
    KZG_HIP_TRY(ctx, hipMemcpyAsync(out_xyzz, ctx->ml[3].p, S * 2 * 128, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KZG_OK;
}

// The one-sum form (the header batch): d_points `count` device-format points and d_w their wire weights, both in the caller's order; the plan
// (of the headers by group) uploaded by locate_upload_plan -> out_xyzz: per segment the XYZZ wire words (16 u64) of sum [w_i] P_i.
// Synchronised on return.  count > 0.
int32_t locate_group_sums_g1_device(kzg_ctx* ctx, const uint4* d_points, const uint4* d_w, const LocatePlan& plan, uint64_t* out_xyzz) {
    RoctxRange range("kzg:locate_group_sums_g1");
    const size_t N = plan.count, S = plan.segs.size(), n_part = plan.part_off.back();
    KZG_HIP_TRY(ctx, ctx->ml[2].reserve(n_part * 4 * NL * 4));
    KZG_HIP_TRY(ctx, ctx->ml[3].reserve(S * 128));
    const uint32_t* d_plan = ctx->ml[1].as<uint32_t>();
    LocateArgs a;
    a.points = d_points; a.n_proofs = 0; a.count = (uint32_t)N;
    a.perm = d_plan; a.seg_of = d_plan + N; a.seg_off = d_plan + 2 * N; a.part_off = d_plan + 2 * N + S + 1;
    a.ci = nullptr; a.w = d_w; a.w2 = nullptr;
    a.partial = ctx->ml[2].as<int32_t>(); a.n_part = (uint32_t)n_part;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_locate_terms<1>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, a);
    KZG_HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_locate_fold<1>), dim3((unsigned)S), dim3(64), 0, ctx->stream, a.partial, a.n_part, a.part_off, ctx->ml[3].as<uint32_t>());
    KZG_HIP_TRY(ctx, hipGetLastError());
    KZG_HIP_TRY(ctx, hipMemcpyAsync(out_xyzz, ctx->ml[3].p, S * 128, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KZG_OK;
}

}  // namespace kzg

#if defined(KZG_DEVICE_BOUND_CHECK)   // the device bound-check variant only (field29.h, `make boundcheck`)
KZG_BOUND_CHECK_EXPORTS(multilocate)
#endif
