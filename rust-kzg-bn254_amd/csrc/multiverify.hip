// multiverify.hip — the Fr side of verifying FK20 coset proofs (multiproof.hip makes them; capi_coset.hip kzg_verify_multiproof_batch checks them):
// N cosets of l values each -> the l coefficients of ONE aggregated interpolation polynomial,
//
//     A_t = sum_i r_i w^(-k_i t) IFFT_l(ys_i)_t,   t < l        (IFFT_l over the root w^m = w_l, natural order in and out, 1 / l included)
//
// where item i is the coset {w^(k_i + j m) : j < l} of the n-point domain, m = n / l, and r_i its weight of the random linear combination.
// I_i(X) = sum_t w^(-k_i t) IFFT_l(ys_i)_t X^t is the polynomial of degree < l through the coset's values, so sum_t A_t [tau^t]_1 is
// [sum_i r_i I_i(tau)]_1: one l-point MSM for the whole batch.  The reference has no coset proofs; for l = 1 this is the
// sum_i r^i y_i of its batch verifier (verifier/src/batch.rs:228-254).
//
// Shapes chosen:
//   * l <= 1024 (k_coset_interp, in coset_kernels.h: multilocate.hip runs its segmented form): one pass over the input, everything else in LDS.  A workgroup of 256 lanes takes tiles of E = 512
//     values (l <= 512: E / l cosets side by side, 512 at l = 1, 32 at l = 16; one butterfly per lane and stage) or E = 1024 (l = 1024:
//     one coset, two butterflies per lane), tile after tile with stride gridDim: unpack (no product: the values stay in the wire
//     residue class a 2^256, the twiddles are internal Montgomery, as in ntt.hip), bit-reversed fill, log l radix-2 stages on 9 limb
//     planes of E words, then entry t times r_i l^-1 w^(-k_i t) and a lazy sum per lane ACROSS tiles in registers.  At the end the
//     E / l columns of a tile are folded by a tree in LDS: one partial row of l sums per workgroup, and k_coset_sum_rows adds the
//     rows (row groups per column, the same tree) and writes canonical wire words.  At most 1 024 workgroups.
//   * w^(-k t): one product of two entries of the factored inverse tables of the n-point domain (ntt_get_tables: 2^10 + n / 2^10
//     entries), exponent k t mod n in 64 bits.  The stage twiddles w_l^-q = w_n^(-q m) come from the same tables, once per workgroup.
//   * l > 1024 (few, long cosets): one ntt_run per coset in place, then k_coset_twist_sum_global, one lane per column.  Not tuned.
//   * mixed shapes (kzg_verify_multiproof_batch_mixed: classes (n_s, l_s) in one batch, A_t summed over the items with l > t): the same tile
//     transform with a workgroup per CLASS (k_coset_interp_mixed), one launch for l <= 512 and one for l = 1024, the per-coset route above
//     1024, and k_coset_sum_rows_mixed over rows of different lengths.  The end of this file; host_coset_mixed.h plans it.
//   * no atomics, no floating point: A_t is an exact field sum, canonical on output, whatever the grid.
// Lazy-reduction bounds are written at each site (the boundcheck build counts violations: tests/test_gpu_multiproof_verify.py).
// Not tried: radix-4 stages (ntt.hip's), a swizzled or padded plane layout (the first stages touch rows 2 b and 2 b + 1 and the fill
// is bit-reversed: 2-way and worse bank conflicts there), wave shuffles for the first six stages, a per-coset w^(-k) power chain in
// place of the table product, more than one tile in flight per workgroup.
// Measured figures: profiles/multiproof_verify.md.
#include "coset_kernels.h"   // MvTables, MvArgs, k_coset_interp and the helpers below its name (shared with multilocate.hip)

#include <algorithm>

namespace kzg {

// out[t] = sum of the `rows` partial rows at column t, canonical wire words.  A workgroup takes cb = min(l, 256) columns with 256 / cb
// row groups, folded by the tree of k_coset_interp.
__global__ void __launch_bounds__(256)
k_coset_sum_rows(const int32_t* __restrict__ partial, uint32_t rows, int log_l, int log_cb, uint4* __restrict__ out) {
    __shared__ int32_t x[NL * 256];
    const uint32_t tid = threadIdx.x, l = 1u << log_l, cb = 1u << log_cb;
    const uint32_t col = blockIdx.x * cb + (tid & (cb - 1)), rg = tid >> log_cb, groups = 256u >> log_cb;
    Fr acc;
    fe_set_zero(acc);
    uint32_t pending = 0;
#pragma unroll 1
    for (uint32_t b = rg; b < rows; b += groups) {
        Fr v;                                                        // a row entry: normalised, in (-m, 2m)
#pragma unroll
        for (int j = 0; j < NL; ++j) v.l[j] = partial[((size_t)b * NL + j) * l + col];
        const bool reduce = ++pending == 32;
        if (reduce) pending = 0;
        mv_lazy_add(acc, v, reduce);
    }
    fe_reduce(acc);
    mv_planes_store(x, 256, tid, acc);
    __syncthreads();
    mv_fold(x, 256, cb, tid);
    if (tid < cb) {
        Fr v;
        mv_planes_load(v, x, 256, tid);
        fe_canon(v);
        uint32_t o[8];
        fe_pack(o, v);
        out[2 * (size_t)col] = make_uint4(o[0], o[1], o[2], o[3]);
        out[2 * (size_t)col + 1] = make_uint4(o[4], o[5], o[6], o[7]);
    }
}

// l > 1024: rows = count x l canonical wire values IFFT_l(ys_i) (ntt_run, 1 / l included); one lane per column t
__global__ void __launch_bounds__(256)
k_coset_twist_sum_global(const uint4* __restrict__ rows, const uint64_t* __restrict__ ks, const uint4* __restrict__ weights, uint32_t count,
                         int log_l, int log_n, MvTables tb, uint4* __restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, l = 1u << log_l;
    if (t >= l) return;
    const uint64_t n_mask = ((uint64_t)1 << log_n) - 1;
    Fr acc, kin;
    fe_set_zero(acc);
#pragma unroll
    for (int j = 0; j < NL; ++j) kin.l[j] = (int32_t)FrParams::K_IN[j];
    uint32_t pending = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < count; ++i) {
        Fr v, s;
        mv_load_words(v, rows + 2 * (((size_t)i << log_l) + t));
        mv_load_words(s, weights + 2 * (size_t)i);
        fe_mul(s, s, kin);
        const uint32_t ex = (uint32_t)((ks[i] * (uint64_t)t) & n_mask);
        if (ex != 0) {
            Fr w;
            mv_root_pow(w, tb, ex);
            fe_mul(s, s, w);
        }
        fe_mul(v, v, s);
        const bool reduce = ++pending == 32;
        if (reduce) pending = 0;
        mv_lazy_add(acc, v, reduce);
    }
    fe_reduce(acc);
    fe_canon(acc);
    uint32_t o[8];
    fe_pack(o, acc);
    out[2 * (size_t)t] = make_uint4(o[0], o[1], o[2], o[3]);
    out[2 * (size_t)t + 1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// Enqueued on ctx->stream, called under ctx->mu with the arguments checked (capi_coset.hip): d_ys count x l wire values (OVERWRITTEN when
// l > 1024), d_ks count indices < n / l, d_weights count wire scalars -> d_out l canonical wire coefficients
int32_t coset_interpolate_rlc_device(kzg_ctx* ctx, uint4* d_ys, const uint64_t* d_ks, const uint4* d_weights, size_t count, size_t n, size_t l, uint4* d_out) {
    RoctxRange range("kzg:coset_interpolate_rlc");
    hipStream_t st = ctx->stream;
    if (count == 0) {
        KZG_HIP_TRY(ctx, hipMemsetAsync(d_out, 0, l * 32, st));
        return KZG_OK;
    }
    const int log_n = __builtin_ctzll(n), log_l = __builtin_ctzll(l);
    NttTables nt;
    int32_t rc = ntt_get_tables(ctx, log_n, true, &nt);
    if (rc != KZG_OK) return rc;
    MvTables tb{nt.lo, nt.hi, nt.lo_len, nt.hi_len, nt.lo_bits};
    if (l > MV_LDS_MAX_L) {
        for (size_t i = 0; i < count; ++i) {
            rc = ntt_run(ctx, d_ys + 2 * i * l, l, true, st, &ctx->mv_ntt);
            if (rc != KZG_OK) return rc;
        }
        hipLaunchKernelGGL(k_coset_twist_sum_global, dim3((unsigned)(l / 256)), dim3(256), 0, st, d_ys, d_ks, d_weights, (uint32_t)count, log_l, log_n, tb, d_out);
        KZG_HIP_TRY(ctx, hipGetLastError());
        return KZG_OK;
    }
    const uint32_t E = l == 1024 ? 1024u : 512u, cpt = E >> log_l;
    const uint32_t tiles = (uint32_t)((count + cpt - 1) / cpt), groups = std::min(tiles, MV_MAX_GROUPS);
    KZG_HIP_TRY(ctx, ctx->mv[3].reserve((size_t)groups * NL * l * 4));
    MvArgs a;
    a.ys = d_ys; a.ks = d_ks; a.weights = d_weights; a.count = (uint32_t)count; a.log_l = log_l; a.log_n = log_n; a.tiles = tiles; a.tb = tb;
    a.partial = ctx->mv[3].as<int32_t>();
    a.rows = nullptr;
    const size_t lds = mv_interp_lds_bytes(E, l);
    if (E == 1024) hipLaunchKernelGGL(k_coset_interp<4>, dim3(groups), dim3(256), lds, st, a);
    else hipLaunchKernelGGL(k_coset_interp<2>, dim3(groups), dim3(256), lds, st, a);
    const int log_cb = std::min(log_l, 8);
    hipLaunchKernelGGL(k_coset_sum_rows, dim3((unsigned)(l >> log_cb)), dim3(256), 0, st, a.partial, groups, log_l, log_cb, d_out);
    KZG_HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

// ---- mixed shapes: classes of different (n, l) into ONE vector of l_max coefficients (host_coset_mixed.h plans, coset_kernels.h has the kernel) ----
// out[t], t < l_max = the field sum of column t over every row that HAS a column t: a row of a class of chunk length l contributes to t < l
// only.  Plane rows (what a workgroup of k_coset_interp_mixed leaves: normalised, in (-m, 2m)) and wire rows (the per-coset route: canonical
// words, so < m, normalised by fe_unpack) enter the same lazy sum, the rule of k_coset_sum_rows: every 32nd sum is reduced (|acc| < 2 m +
// 32 * 2 m = 66 m < 169 m), the others normalised; a lane counts the sums it makes.  No atomics, no floating point: an exact field sum,
// canonical on output, whatever the rows' order.  A workgroup takes cb = min(l_max, 256) columns with 256 / cb row groups.
__global__ void __launch_bounds__(256)
k_coset_sum_rows_mixed(const int32_t* __restrict__ partial, const uint4* __restrict__ wire_rows, const kzg_host::MixedRow* __restrict__ rows, uint32_t n_rows,
                       int log_cb, uint4* __restrict__ out) {
    __shared__ int32_t x[NL * 256];
    const uint32_t tid = threadIdx.x, cb = 1u << log_cb;
    const uint32_t col = blockIdx.x * cb + (tid & (cb - 1)), rg = tid >> log_cb, groups = 256u >> log_cb;
    Fr acc;
    fe_set_zero(acc);
    uint32_t pending = 0;
#pragma unroll 1
    for (uint32_t b = rg; b < n_rows; b += groups) {
        const kzg_host::MixedRow r = rows[b];
        const uint32_t l = 1u << (r.log_l_kind & 0xFFu);
        if (col >= l) continue;
        Fr v;
        if (r.log_l_kind & 0x100u) {
            mv_load_words(v, wire_rows + 2 * ((size_t)r.off + col));
        } else {
#pragma unroll
            for (int j = 0; j < NL; ++j) v.l[j] = partial[(size_t)r.off + (size_t)j * l + col];
        }
        const bool reduce = ++pending == 32;
        if (reduce) pending = 0;
        mv_lazy_add(acc, v, reduce);
    }
    fe_reduce(acc);                                                  // |acc| < 66 m -> (-m, 2m), normalised
    mv_planes_store(x, 256, tid, acc);
    __syncthreads();
    mv_fold(x, 256, cb, tid);
    if (tid < cb) {
        Fr v;
        mv_planes_load(v, x, 256, tid);
        fe_canon(v);
        uint32_t o[8];
        fe_pack(o, v);
        out[2 * (size_t)col] = make_uint4(o[0], o[1], o[2], o[3]);
        out[2 * (size_t)col + 1] = make_uint4(o[4], o[5], o[6], o[7]);
    }
}

// Enqueued on ctx->stream, called under ctx->mu with the arguments checked (capi_coset.hip) and the plan's tables on the device (t): d_ys the
// ragged wire values in the caller's order (an item of l > 1024 is OVERWRITTEN by its transform), d_ks / d_weights in the caller's order ->
// d_out p.l_max canonical wire coefficients.  Launch groups by chunk length: the classes of l <= 512 in one launch of the 512-value tile,
// those of l = 1024 in a second launch of the 1024-value tile, an item of l > 1024 through ntt_run and k_coset_twist_sum_global (count = 1:
// its twisted, weighted transform) into a wire row of its own; then ONE k_coset_sum_rows_mixed over all rows.  Rows live in ctx->mv[3].
int32_t coset_interpolate_rlc_mixed_device(kzg_ctx* ctx, const kzg_host::MixedPlan& p, uint4* d_ys, const uint64_t* d_ks, const uint4* d_weights,
                                           const MixedDevTables& t, uint4* d_out) {
    RoctxRange range("kzg:coset_interpolate_rlc_mixed");
    hipStream_t st = ctx->stream;
    if (p.count == 0) {
        if (p.l_max) KZG_HIP_TRY(ctx, hipMemsetAsync(d_out, 0, p.l_max * 32, st));
        return KZG_OK;
    }
    const size_t plane_bytes = (p.plane_words * 4 + 31) & ~(size_t)31;
    KZG_HIP_TRY(ctx, ctx->mv[3].reserve(std::max<size_t>(plane_bytes + p.wire_elems * 32, 32)));
    int32_t* d_partial = ctx->mv[3].as<int32_t>();
    uint4* d_wire = reinterpret_cast<uint4*>(ctx->mv[3].as<uint8_t>() + plane_bytes);
    if (!p.wg_class[0].empty() || !p.wg_class[1].empty()) {
        NttTables nt;
        int32_t rc = ntt_get_tables(ctx, p.log_n_max, true, &nt);
        if (rc != KZG_OK) return rc;
        MvMixedArgs a;
        a.ys = d_ys; a.ks = d_ks; a.weights = d_weights; a.perm = t.perm; a.val_off = t.val_off;
        a.classes = static_cast<const kzg_host::MixedClassDev*>(t.classes);
        a.log_n_max = p.log_n_max;
        a.tb = MvTables{nt.lo, nt.hi, nt.lo_len, nt.hi_len, nt.lo_bits};
        a.partial = d_partial;
        if (!p.wg_class[0].empty()) {
            a.wg_class = t.wg_class[0];
            hipLaunchKernelGGL(k_coset_interp_mixed<2>, dim3((unsigned)p.wg_class[0].size()), dim3(256), p.lds_bytes[0], st, a);
        }
        if (!p.wg_class[1].empty()) {
            a.wg_class = t.wg_class[1];
            hipLaunchKernelGGL(k_coset_interp_mixed<4>, dim3((unsigned)p.wg_class[1].size()), dim3(256), p.lds_bytes[1], st, a);
        }
        KZG_HIP_TRY(ctx, hipGetLastError());
    }
    for (const kzg_host::MixedLongItem& it : p.long_items) {
        const size_t l = (size_t)1 << it.log_l;
        NttTables nt;
        int32_t rc = ntt_get_tables(ctx, (int)it.log_n, true, &nt);
        if (rc != KZG_OK) return rc;
        uint4* vals = d_ys + 2 * (size_t)it.val_off;
        rc = ntt_run(ctx, vals, l, true, st, &ctx->mv_ntt);
        if (rc != KZG_OK) return rc;
        hipLaunchKernelGGL(k_coset_twist_sum_global, dim3((unsigned)(l / 256)), dim3(256), 0, st, vals, d_ks + it.item, d_weights + 2 * (size_t)it.item, 1u,
                           (int)it.log_l, (int)it.log_n, MvTables{nt.lo, nt.hi, nt.lo_len, nt.hi_len, nt.lo_bits}, d_wire + 2 * (size_t)it.row_off);
        KZG_HIP_TRY(ctx, hipGetLastError());
    }
    int log_cb = 0;
    while (((size_t)1 << log_cb) < p.l_max && log_cb < 8) ++log_cb;
    hipLaunchKernelGGL(k_coset_sum_rows_mixed, dim3((unsigned)(p.l_max >> log_cb)), dim3(256), 0, st, d_partial, d_wire,
                       static_cast<const kzg_host::MixedRow*>(t.rows), (uint32_t)p.rows.size(), log_cb, d_out);
    KZG_HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

}  // namespace kzg

#if defined(KZG_DEVICE_BOUND_CHECK)   // the device bound-check variant only (field29.h, `make boundcheck`)
KZG_BOUND_CHECK_EXPORTS(multiverify)
#endif
