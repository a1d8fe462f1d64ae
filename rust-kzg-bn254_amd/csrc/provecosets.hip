// provecosets.hip — the values and the proofs of SELECTED cosets of polynomials the caller holds (kzg_prove_cosets, kzg_coset_quotients;
// capi_prove.hip), without the FK20 pipeline that computes every proof.  The conventions are the encoder's (multiproof.hip): w the library's
// primitive n-th root, coset k < m = n / l is {w^(k + j m) : j < l}, c = w^(k l), the proof is [q(tau)]_1 with f = q (X^l - c) + r.
//
// An ITEM is a (polynomial, coset) pair.  Per item and residue rho < l the coefficients f_(rho + t l), t < D = d / l, are one chain of the
// suffix Horner recurrence G_t = f_(rho + t l) + c G_(t+1); the quotient is q_(rho + (t-1) l) = G_t and the remainder r_rho = G_0
// (host_prove_cosets.h has the derivation, the segment identity and the plan).  Three kinds of pass, every lane at most S dependent products:
//   k_pc_local   one lane per (item, rho, segment): the segment's own Horner sum loc_t into the quotient row, its head into the heads;
//                run again on the heads of the level below with the multiplier c^(S^level) until a level is one segment
//   k_pc_fix     one lane per element of a level >= 1: loc + c_i^(..) carry, top level down
//   k_pc_fix0    one lane per element of the quotient row: q = loc + c^(..) carry; lane t = 0 writes the row's zero at rho + (D-1) l and
//                the twisted remainder r_rho w^(k rho)
// The values are y_j = sum_rho (r_rho w^(k rho)) (w^m)^(j rho): one l-point forward NTT per item, all items of a group as the rows of one
// ntt_run_batch.  The proofs are the commitments of the quotient rows (d coefficients each, the top l zero) over the first d points of the
// SRS: one commit_batch_device per group, or msm_run for a group of one item (ProveCosetsPlan::msm_single).
// Elements travel between the passes as canonical wire words (wire_load / wire_store): every output is a function of the value alone, so
// the rows are those of the encoder bit for bit.  The Fr work is ~3 d products per item against an MSM of d terms: the kernels are plain.
// Lazy-reduction bounds are written at each site; the boundcheck build counts violations (tests/test_gpu_prove_cosets.py).
// Not tried: a wave-shuffle affine scan in place of the carry recursion, limb planes instead of wire words between the passes, skipping
// the zero tail of a polynomial, overlapping a group's downloads with the next group's kernels.  Measured figures: profiles/prove_cosets.md.
#include "poly_common.h"
#include "host_prove_cosets.h"

#include <algorithm>
#include <numeric>
#include <vector>

namespace kzg {

struct PcArgs {
    const uint4* src;           // level 0: the polynomials (coefficients), src_stride elements apart, row item_poly[item]; level >= 1: the level's elements, row `item`
    size_t src_stride;
    uint4* dst;                 // where loc_t goes: level 0 the quotient rows (pc_quot_elem; nullptr: not kept), level >= 1 == src (in place)
    size_t dst_stride;
    uint4* heads;               // local pass: the segment heads it writes (nullptr: none); fix-up: the final values of the level above
    size_t heads_stride;
    const uint32_t* item_poly;
    const uint32_t* item_k;
    uint32_t len, nseg, l, n_mask;
    int log_l, log_S, shift, level0;
    NttTables tb;               // forward tables of the n-point domain
};

// lane (rho, seg) of item blockIdx.y: loc_t for t in [seg S, min((seg + 1) S, len)), downwards
__global__ void __launch_bounds__(256)
k_pc_local(PcArgs a) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a.nseg * a.l) return;
    const uint32_t rho = x & (a.l - 1), seg = x >> a.log_l, item = blockIdx.y;
    const uint4* src = a.src + 2 * (size_t)(a.level0 ? a.item_poly[item] : item) * a.src_stride;
    uint4* dst = a.dst ? a.dst + 2 * (size_t)item * a.dst_stride : nullptr;
    Fr c, acc;
    domain_elem(c, a.tb, pc_mult_exp(a.item_k[item], a.shift, a.n_mask));       // (-m, 2m), normalised
    fe_set_zero(acc);
    const uint32_t lo = seg << a.log_S, hi = min(lo + (1u << a.log_S), a.len);
#pragma unroll 1
    for (uint32_t j = hi; j-- > lo;) {
        Fr f, t;
        wire_load(f, src, pc_elem(j, a.l, rho));                                   // (-m, 2m)
        fe_mul(t, c, acc);                                                         // |c acc| < 2m 4m; (-m, 2m)
        fe_add(acc, t, f);
        fe_norm(acc);                                                              // (-2m, 4m), normalised
        if (dst && (j > 0 || !a.level0)) wire_store(dst, a.level0 ? pc_quot_elem(j, a.l, rho) : pc_elem(j, a.l, rho), acc);
    }
    if (a.heads) wire_store(a.heads + 2 * (size_t)item * a.heads_stride, pc_elem(seg, a.l, rho), acc);
}

// level >= 1, lane (rho, j) of item blockIdx.y: G_j = loc_j + c_i^((seg + 1) S - j) G'_(seg + 1) with G' the level above (a.heads), in place
__global__ void __launch_bounds__(256)
k_pc_fix(PcArgs a) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a.len * a.l) return;
    const uint32_t rho = x & (a.l - 1), j = x >> a.log_l, seg = j >> a.log_S, item = blockIdx.y;
    if (seg + 1 >= a.nseg) return;                                                 // the last segment has no carry
    uint4* data = a.dst + 2 * (size_t)item * a.dst_stride;
    Fr w, carry, loc, t;
    domain_elem(w, a.tb, pc_pow_exp(a.item_k[item], a.shift, ((seg + 1) << a.log_S) - j, a.n_mask));
    wire_load(carry, a.heads + 2 * (size_t)item * a.heads_stride, pc_elem(seg + 1, a.l, rho));
    wire_load(loc, data, pc_elem(j, a.l, rho));
    fe_mul(t, w, carry);                                                           // (-m, 2m)
    fe_add(t, t, loc);
    fe_norm(t);                                                                    // (-2m, 4m)
    wire_store(data, pc_elem(j, a.l, rho), t);
}

// level 0, lane (rho, t) of item blockIdx.y (only t = 0 when no quotient row is kept): the quotient row's final words, its zero, the twisted remainder
__global__ void __launch_bounds__(256)
k_pc_fix0(PcArgs a, uint4* rem /* n_items x l, or nullptr */) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= (a.dst ? a.len : 1u) * a.l) return;
    const uint32_t rho = x & (a.l - 1), t = x >> a.log_l, item = blockIdx.y, k = a.item_k[item];
    uint4* row = a.dst ? a.dst + 2 * (size_t)item * a.dst_stride : nullptr;
    const uint4* heads = a.heads + 2 * (size_t)item * a.heads_stride;
    if (t == 0) {
        if (rem) {
            Fr r, w, y;
            wire_load(r, heads, pc_elem(0, a.l, rho));                             // G_0, final
            domain_elem(w, a.tb, pc_twist_exp(k, rho, a.n_mask));
            fe_mul(y, r, w);
            wire_store(rem + 2 * (size_t)item * a.l, rho, y);
        }
        if (row) {
            const size_t top = pc_elem(a.len - 1, a.l, rho);                       // q_(rho + (D-1) l) = G_D = 0
            row[2 * top] = make_uint4(0, 0, 0, 0);
            row[2 * top + 1] = make_uint4(0, 0, 0, 0);
        }
        return;
    }
    const uint32_t seg = t >> a.log_S;
    if (seg + 1 >= a.nseg) return;                                                 // loc is final and canonical already
    Fr w, carry, loc, s;
    domain_elem(w, a.tb, pc_pow_exp(k, a.shift, ((seg + 1) << a.log_S) - t, a.n_mask));
    wire_load(carry, heads, pc_elem(seg + 1, a.l, rho));
    wire_load(loc, row, pc_quot_elem(t, a.l, rho));
    fe_mul(s, w, carry);
    fe_add(s, s, loc);
    fe_norm(s);                                                                    // (-2m, 4m)
    wire_store(row, pc_quot_elem(t, a.l, rho), s);
}

static inline unsigned pc_grid(size_t threads) { return (unsigned)((threads + 255) / 256); }

// The Fr passes of a group of g items whose indices are uploaded (d_poly, d_k): quotient rows at q (nullptr: not kept), heads block at
// heads, twisted remainders at rem (nullptr: no values).  Enqueued on st.
static int32_t pc_enqueue_passes(kzg_ctx* ctx, hipStream_t st, const ProveCosetsPlan& p, const NttTables& tb, const uint4* polys, size_t g,
                                 const uint32_t* d_poly, const uint32_t* d_k, uint4* q, uint4* heads, uint4* rem) {
    const unsigned gy = (unsigned)g;
    PcArgs a{};
    a.item_poly = d_poly; a.item_k = d_k;
    a.l = (uint32_t)p.l; a.n_mask = (uint32_t)(p.n - 1); a.log_l = p.log_l; a.log_S = p.log_S; a.tb = tb;
    a.heads_stride = p.heads_elems;
    for (int i = 0; i < p.n_levels; ++i) {                                         // local passes, level 0 up
        const ProveLevel& L = p.level[i];
        a.level0 = i == 0;
        a.len = L.len; a.nseg = L.nseg; a.shift = L.shift;
        if (i == 0) { a.src = polys; a.src_stride = p.d; a.dst = q; a.dst_stride = p.d; }
        else { a.src = heads + 2 * L.data_off; a.src_stride = p.heads_elems; a.dst = heads + 2 * L.data_off; a.dst_stride = p.heads_elems; }
        a.heads = L.heads ? heads + 2 * L.heads_off : nullptr;
        hipLaunchKernelGGL(k_pc_local, dim3(pc_grid((size_t)L.nseg * p.l), gy), dim3(256), 0, st, a);
    }
    for (int i = p.n_levels - 2; i >= 1; --i) {                                    // fix-ups above level 0, top down
        const ProveLevel& L = p.level[i];
        a.level0 = 0;
        a.len = L.len; a.nseg = L.nseg; a.shift = L.shift;
        a.src = nullptr; a.src_stride = 0;
        a.dst = heads + 2 * L.data_off; a.dst_stride = p.heads_elems;
        a.heads = heads + 2 * L.heads_off;
        hipLaunchKernelGGL(k_pc_fix, dim3(pc_grid((size_t)L.len * p.l), gy), dim3(256), 0, st, a);
    }
    const ProveLevel& L0 = p.level[0];
    a.level0 = 1;
    a.len = L0.len; a.nseg = L0.nseg; a.shift = L0.shift;
    a.src = nullptr; a.src_stride = 0;
    a.dst = q; a.dst_stride = p.d;
    a.heads = heads + 2 * L0.heads_off;
    hipLaunchKernelGGL(k_pc_fix0, dim3(pc_grid(q ? p.d : p.l), gy), dim3(256), 0, st, a, rem);
    KZG_HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

// rows of `row` u64 words: out[order[i0 + i]] = staged[i]
static void pc_scatter_rows(uint64_t* out, const uint64_t* staged, const size_t* order, size_t g, size_t row) {
    for (size_t i = 0; i < g; ++i) memcpy(out + order[i] * row, staged + i * row, row * 8);
}

// called under ctx->mu with the device set, the arguments checked and planned, n_items > 0 and slot 0 idle (capi_prove.hip).  srs: only
// with out_xy.  Synchronised on return.
int32_t prove_cosets_run(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* polys_mont, size_t count, bool eval_form, const ProveCosetsPlan& p,
                         const uint64_t* poly_indices, const uint64_t* coset_indices, uint64_t* out_q, uint64_t* out_ys, uint64_t* out_xy, uint8_t* out_inf) {
    RoctxRange range("kzg:prove_cosets");
    const size_t d = p.d, l = p.l, n_items = p.n_items;
    hipStream_t st = ctx->stream;
    // the items ordered by polynomial (stable): the items of one blob re-read its coefficients from the cache
    std::vector<size_t> order(n_items);
    std::iota(order.begin(), order.end(), (size_t)0);
    bool in_order = true;
    if (poly_indices) {
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return poly_indices[x] < poly_indices[y]; });
        for (size_t i = 0; i < n_items; ++i) in_order &= order[i] == i;
    }
    // the referenced polynomials, compact, in ascending order: runs of neighbours go up as one copy; eval form: one batched inverse NTT
    std::vector<uint32_t> slot_of(count, NO_INDEX);
    size_t n_ref = 0;
    for (size_t i = 0; i < n_items; ++i) {
        const size_t b = poly_indices ? (size_t)poly_indices[order[i]] : 0;
        if (slot_of[b] == NO_INDEX) slot_of[b] = (uint32_t)n_ref++;
    }
    KZG_HIP_TRY(ctx, ctx->pc[0].reserve(n_ref * d * 32));
    uint4* polys = ctx->pc[0].as<uint4>();
    for (size_t b = 0; b < count;) {
        if (slot_of[b] == NO_INDEX) { ++b; continue; }
        size_t e = b + 1;
        while (e < count && slot_of[e] != NO_INDEX) ++e;                           // (slots ascend with the index: a run is contiguous on both sides)
        KZG_HIP_TRY(ctx, hipMemcpyAsync(polys + 2 * (size_t)slot_of[b] * d, polys_mont + b * d * 4, (e - b) * d * 32, hipMemcpyHostToDevice, st));
        b = e;
    }
    int32_t rc = KZG_OK;
    if (eval_form) { rc = ntt_run_batch(ctx, polys, d, n_ref, true, st, &ctx->pc_ntt); if (rc != KZG_OK) return rc; }
    NttTables tb;
    rc = ntt_get_tables(ctx, p.log_n, false, &tb);
    if (rc != KZG_OK) return rc;
    const size_t G = p.group;
    KZG_HIP_TRY(ctx, ctx->pc[1].reserve(p.quotients ? G * d * 32 : 0));
    KZG_HIP_TRY(ctx, ctx->pc[2].reserve(G * (p.heads_elems + (p.values ? l : 0)) * 32));
    KZG_HIP_TRY(ctx, ctx->pc[3].reserve(G * PROVE_ITEM_INDEX_BYTES));
    uint4* q = p.quotients ? ctx->pc[1].as<uint4>() : nullptr;
    uint4* heads = ctx->pc[2].as<uint4>();
    uint4* rem = p.values ? heads + 2 * G * p.heads_elems : nullptr;
    uint32_t* d_poly = ctx->pc[3].as<uint32_t>();
    uint32_t* d_k = d_poly + G;
    std::vector<uint32_t> idx(2 * G);
    std::vector<uint64_t> staged;                                                  // a group's rows in group order, when the caller's order differs
    std::vector<uint8_t> staged_inf;
    for (size_t i0 = 0; i0 < n_items; i0 += G) {
        const size_t g = std::min(G, n_items - i0);
        for (size_t i = 0; i < g; ++i) {
            const size_t it = order[i0 + i];
            idx[i] = slot_of[poly_indices ? (size_t)poly_indices[it] : 0];
            idx[G + i] = (uint32_t)coset_indices[it];
        }
        KZG_HIP_TRY(ctx, hipMemcpyAsync(d_poly, idx.data(), 2 * G * 4, hipMemcpyHostToDevice, st));
        rc = pc_enqueue_passes(ctx, st, p, tb, polys, g, d_poly, d_k, q, heads, rem);
        if (rc != KZG_OK) return rc;
        if (out_ys) {
            rc = ntt_run_batch(ctx, rem, l, g, false, st, &ctx->pc_ntt);           // l = 1: y = r_0, nothing to transform
            if (rc != KZG_OK) return rc;
            uint64_t* dst = out_ys + i0 * l * 4;
            if (!in_order) { staged.resize(g * l * 4); dst = staged.data(); }
            KZG_HIP_TRY(ctx, hipMemcpyAsync(dst, rem, g * l * 32, hipMemcpyDeviceToHost, st));
            KZG_HIP_TRY(ctx, hipStreamSynchronize(st));
            if (!in_order) pc_scatter_rows(out_ys, staged.data(), order.data() + i0, g, l * 4);
        }
        if (out_q) {
            uint64_t* dst = out_q + i0 * d * 4;
            if (!in_order) { staged.resize(g * d * 4); dst = staged.data(); }
            KZG_HIP_TRY(ctx, hipMemcpyAsync(dst, q, g * d * 32, hipMemcpyDeviceToHost, st));
            KZG_HIP_TRY(ctx, hipStreamSynchronize(st));
            if (!in_order) pc_scatter_rows(out_q, staged.data(), order.data() + i0, g, d * 4);
        }
        if (out_xy) {
            KZG_HIP_TRY(ctx, hipStreamSynchronize(st));                            // the batched commitments run on the slots' streams: the rows are complete
            uint64_t* xy = out_xy + i0 * 8;
            uint8_t* inf = out_inf + i0;
            if (!in_order) { staged.resize(g * 8); staged_inf.resize(g); xy = staged.data(); inf = staged_inf.data(); }
            if (g == 1 && p.msm_single) rc = msm_run(ctx, srs_bases(srs, 0, d, ctx->msm_c_override == 0), q, d, xy, inf, nullptr);
            else rc = commit_batch_device(ctx, srs, q, d, g, xy, inf);
            if (rc != KZG_OK) return rc;
            if (!in_order) {
                pc_scatter_rows(out_xy, staged.data(), order.data() + i0, g, 8);
                for (size_t i = 0; i < g; ++i) out_inf[order[i0 + i]] = staged_inf[i];
            }
        }
        KZG_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return KZG_OK;
}

}  // namespace kzg

#if defined(KZG_DEVICE_BOUND_CHECK)   // the device bound-check variant only (field29.h, `make boundcheck`)
#include "field29.h"
KZG_BOUND_CHECK_EXPORTS(provecosets)
#endif
