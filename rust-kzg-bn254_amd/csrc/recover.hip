// recover.hip — erasure decoding (kzg_recover_from_cosets, kzg_recover_from_cosets_batch, capi_verify.hip): from the values of `count` of the m = n / l cosets
// {w^(k + j m) : j < l} of the n-point domain to the polynomial f of degree < count l through them, as n coefficients or n evaluations.
// The reference has no coset code; the conventions are those of multiproof.hip and multiverify.hip.
//
// With M the missing cosets, z(Y) = prod_{k in M} (Y - w^(l k)) (a polynomial over the m-th roots w^l) and Z(X) = z(X^l), Z vanishes
// exactly on the missing cosets, so D_i = f(w^i) Z(w^i) is known everywhere: the value times z(w^(l k)) on a present coset k = i mod m,
// zero on a missing one.  deg f Z < count l + l |M| = n, so IFFT_n(D) is f Z exactly, and f is its quotient by Z taken on the shifted
// domain {g w^i}, g = 5, where Z(g w^i) = z(s w^(l i)), s = g^l, has no zero (s is not an m-th root of unity: g^n != 1):
//   1. k_recover_vanish / k_recover_vanish_fold   z on the m points w^(l p) and on the m points s w^(l p); the latter inverted
//   2. k_recover_scatter                          D (every position written once: no memset, no index of the caller reaches a store)
//   3. ntt_run_batch inverse                      P = f Z
//   4. k_recover_scale<0>, ntt_run_batch forward  P_t g^t -> P(g w^i)
//   5. k_recover_scale<1>                         / z(s w^(l (i mod m)))  -> f(g w^i)
//   6. ntt_run_batch inverse, k_recover_scale<2>  g^-t -> the coefficients of f; a word of flags ORs "a coefficient from degree_bound on is not zero"
//   7. ntt_run_batch forward                      when evaluations are asked for
// ONE set of kernels serves both entries.  A call works through its blobs in groups (host_recover.h: RecoverBatchPlan); inside a group every
// stage above is one launch: scatter, the scale passes and the transforms take the blob as grid.y (one flag word per blob), the vanishing
// values take the PATTERN -- a distinct missing set of the group -- as a grid dimension, with one missing list and one zdom / zsinv / partial
// region per pattern, and blob b reads the item map of its index row and the values of pattern_of[b].  The split of M aims all patterns
// together at RECOVER_TARGET_GROUPS workgroups (recover_vanish_split).  The single call is the group of one blob, one index row, one pattern:
// the same launches with grid.y = grid.z = 1 as before the batch existed, one small upload instead of two.  Per group: one upload of the values,
// one of item maps + patterns + missing lists, one download of the rows, one of the flags, one synchronisation.  With one index row for all
// blobs the later groups of a call reuse the first group's upload and vanishing values.  Rows shorter than n (coefficients, out_len < n) are
// compacted by k_recover_scale<2> into the transforms' scratch, dead by then, so the download stays one contiguous copy (a strided 2-D copy
// from the work rows was the alternative; not measured).
// Shapes chosen:
//   * the vanishing values are DIRECT products, 2 m |M| field products (no coefficient form of z, no product tree): one lane per output
//     point keeps a running product over tiles of 256 roots, staged in LDS as 9 limb planes (every lane reads the same root: an LDS
//     broadcast).  The roots w_n^(l k) come from the forward tables of the n-point domain (ntt_get_tables).  2 m / 256 workgroups do not
//     fill the device below m = 2^17, so M is split across blockIdx.y into up to RECOVER_TARGET_GROUPS workgroups in all and the fold multiplies
//     the partial products: a field product, the same element whatever the split, and canonical words leave the call.
//   * the m divisors are inverted once: Montgomery's trick per workgroup of 256 (product tree in LDS, one fe_inverse_safegcd: lds_tree_invert).
//   * g^t and g^-t are factored like the twiddle tables, 2^10 + n / 2^10 entries each (one product per element from 2^10 on), kept per context.
//   * values stay in the wire residue class a 2^256 between the kernels (the factors are internal Montgomery), as in ntt.hip; every kernel
//     writes canonical words, so equal inputs give equal bits.
// SERIALIZED FORM (kzg_recover_from_cosets_batch_bytes, kzg_retrieve_blobs_bytes): the same driver takes its values as 32-byte big-endian
// integers and writes its rows as such (RecoverIo, engine.h).  The values are decoded ON LOAD by k_recover_scatter<true>: every present
// value is read exactly once there, so the decode is a byte swap, a compare with r and one product into the wire class in front of the
// product with zdom -- no pass of its own over count l 32 B per blob (k_fr_decode_be in place over the staged bytes was the alternative).
// The fused load keeps the kernel free of scratch (the compiler's figures: profiles/recover_bytes.md).  A value >= r computes with zero
// and reports atomicMin(bad, value index << 2) on one word per call, read with the group's flags at the group's one synchronisation;
// the call stops at the first group with a bad value (groups are in order: it holds the smallest bad index of the call), and rows of
// that group and of EARLIER groups may already have been written to the caller's buffer (flags: of earlier groups only).  Coefficient rows leave through fr_encode_wire_to_be in
// k_recover_scale<2, true>; evaluation rows get one in-place pass k_fr_encode_be behind the last transform.  The values may also be
// device-resident (words or bytes): no upload at all, the scatter reads them where they lie.
// Lazy-reduction bounds are written at each site; the boundcheck build counts violations (tests/test_gpu_recover.py, tests/test_gpu_recover_batch.py,
// tests/test_gpu_recover_bytes.py).
// Not tried: the scale passes fused into the first load / last store of the transforms next to them, two running products per lane
// (fe_mul2), a product tree for m > 2^16, the complement form z = (Y^m - 1) / prod_present, pinned staging, one group's copies behind the next group's kernels.  Measured figures: profiles/recover.md,
// profiles/recover_batch.md.
#include "poly_common.h"
#include "fe_invert.h"
#include "g1_decode.h"   // the steps of fr_decode_be_to_wire on load, fr_encode_wire_to_be on store

#include <algorithm>

namespace kzg {

constexpr uint32_t RC_THREADS = RECOVER_THREADS;   // 256 (host_recover.h: the workspace of a group depends on the geometry)
constexpr uint32_t RC_TILE = RECOVER_TILE;         // roots per LDS tile: one per lane to stage
constexpr int RC_LO_BITS = 10;                     // g^t = glo[t & 1023] ghi[t >> 10]
constexpr uint32_t RC_LO_LEN = 1u << RC_LO_BITS;
static_assert(NL == RECOVER_LIMBS && RC_TILE == RC_THREADS, "host_recover.h sizes the limb planes; one lane stages one root");

struct RcPow { const int32_t* lo; const int32_t* hi; uint32_t hi_len; };

// the 256-bit words of a wire element as limbs, no product: < 2^256 < 5.3 m, normalised
__device__ __forceinline__ void rc_load_words(Fr& v, const uint4* __restrict__ p, size_t i) {
    const uint4 lo = p[2 * i], hi = p[2 * i + 1];
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    fe_unpack(v, w);
}
// v canonical -> its words
__device__ __forceinline__ void rc_store_words(uint4* __restrict__ p, size_t i, const Fr& v) {
    uint32_t o[8];
    fe_pack(o, v);
    p[2 * i] = make_uint4(o[0], o[1], o[2], o[3]);
    p[2 * i + 1] = make_uint4(o[4], o[5], o[6], o[7]);
}
// v normalised in (-m, 2m) -> canonical words
__device__ __forceinline__ void rc_store_canon(uint4* __restrict__ p, size_t i, Fr& v) {
    fe_canon(v);
    rc_store_words(p, i, v);
}
// g^(+-t), t < 2^10 hi_len, from the factored table: in (-m, 2m), normalised
__device__ __forceinline__ void rc_gpow(Fr& w, const RcPow& t, uint32_t e) {
    pl_load(w, t.lo, RC_LO_LEN, e & (RC_LO_LEN - 1));
    const uint32_t eh = e >> RC_LO_BITS;
    if (eh != 0) {
        Fr h;
        pl_load(h, t.hi, t.hi_len, eh);
        fe_mul(w, w, h);
    }
}

// ---- the power tables: planes[9][len] of g^(t step) (inverse: g^-(t step)), internal form; once per context and size ----------------
__global__ void __launch_bounds__(RC_THREADS)
k_recover_gpow_table(int32_t* __restrict__ planes, uint32_t len, uint32_t step, int inverse) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= len) return;
    Fr one, base, acc;
    fe_set_one(one);
    fe_add(base, one, one);                                       // 1 + 1, limbs < 2^30
    fe_dbl(base, base);                                           // 4: limbs < 2^31
    fe_norm(base);
    fe_add(base, base, one);
    fe_reduce(base);                                              // 5 in (-m, 2m) (|5 * 1| < 5 m)
    if (inverse) { Fr b = base; fe_inverse_safegcd(base, b); }
    fe_set_one(acc);
    for (uint32_t e = t * step; e; e >>= 1) {                     // t step < 2^24
        if (e & 1u) fe_mul(acc, acc, base);
        fe_sqr(base, base);
    }
    pl_store(planes, len, t, acc);
}

// ---- 1. vanishing values ---------------------------------------------------------------------------------------------------------------
struct RcVanishArgs {
    const uint32_t* missing;    // gridDim.z patterns of |M| coset indices < m, each ascending
    uint32_t n_missing, per_split;
    uint32_t m;
    int log_l;
    NttTables tb;               // forward tables of the n-point domain
    RcPow gp;                   // g^t
    int32_t* partial;           // per pattern: gridDim.y rows of 9 planes of 2 m words
};
// lane p < 2 m of row blockIdx.y of pattern blockIdx.z: prod over the row's slice of M of (x_p - w^(l k)), x_p = w^(l p) (p < m) or
// g^l w^(l (p - m)).  An empty slice (M empty) gives 1.
__global__ void __launch_bounds__(RC_THREADS)
k_recover_vanish(RcVanishArgs a) {
    __shared__ int32_t roots[NL * RC_TILE];
    const uint32_t tid = threadIdx.x, p = blockIdx.x * RC_THREADS + tid, two_m = 2 * a.m;
    const uint32_t* __restrict__ missing = a.missing + (size_t)blockIdx.z * a.n_missing;
    int32_t* __restrict__ partial = a.partial + (size_t)blockIdx.z * NL * gridDim.y * two_m;
    const uint32_t first = blockIdx.y * a.per_split, last = min(a.n_missing, first + a.per_split);
    Fr x, acc;
    fe_set_one(acc);
    fe_set_zero(x);
    if (p < two_m) {
        const uint32_t q = p < a.m ? p : p - a.m;
        domain_elem(x, a.tb, q << a.log_l);                          // q l < n
        if (p >= a.m) {
            Fr s;
            rc_gpow(s, a.gp, 1u << a.log_l);                         // l <= n / 2: inside the table
            fe_mul(x, x, s);
        }
    }
#pragma unroll 1
    for (uint32_t base = first; base < last; base += RC_TILE) {      // uniform across the workgroup
        const uint32_t cnt = min(RC_TILE, last - base);
        if (tid < cnt) {
            Fr w;
            domain_elem(w, a.tb, missing[base + tid] << a.log_l);
            pl_store(roots, RC_TILE, tid, w);
        }
        __syncthreads();
#pragma unroll 1
        for (uint32_t r = 0; r < cnt; ++r) {
            Fr w, d;
            pl_load(w, roots, RC_TILE, r);
            fe_sub(d, x, w);                                         // both normalised in (-m, 2m): limbs within +-2^29, |d| < 3 m
            fe_mul(acc, acc, d);                                     // |acc d| < 2 m * 3 m
        }
        __syncthreads();                                             // the next tile overwrites the roots
    }
    if (p < two_m) pl_store(partial, (size_t)gridDim.y * two_m, (size_t)blockIdx.y * two_m + p, acc);
}

// lane p < 2 m of pattern blockIdx.y: the product of its `rows` partial products; p < m: stored (zdom[p] = z(w^(l p))); p >= m: inverted, Montgomery's trick per
// workgroup (lds_tree_invert), zsinv[p - m] = 1 / z(s w^(l (p - m))).  No divisor is zero.
__global__ void __launch_bounds__(RC_THREADS)
k_recover_vanish_fold(const int32_t* __restrict__ partial, uint32_t rows, uint32_t m, int32_t* __restrict__ zdom, int32_t* __restrict__ zsinv) {
    __shared__ int32_t tree[NL * 2 * RC_THREADS];                    // heap order: root 1, leaves RC_THREADS + t
    constexpr uint32_t Lf = RC_THREADS, S = 2 * RC_THREADS;
    const uint32_t t = threadIdx.x, p = blockIdx.x * RC_THREADS + t, two_m = 2 * m;
    partial += (size_t)blockIdx.y * NL * rows * two_m;
    zdom += (size_t)blockIdx.y * NL * m;
    zsinv += (size_t)blockIdx.y * NL * m;
    Fr v;
    fe_set_one(v);
    if (p < two_m) {
        pl_load(v, partial, (size_t)rows * two_m, p);
        for (uint32_t b = 1; b < rows; ++b) {
            Fr u;
            pl_load(u, partial, (size_t)rows * two_m, (size_t)b * two_m + p);
            fe_mul(v, v, u);                                         // both in (-m, 2m)
        }
        if (p < m) pl_store(zdom, m, p, v);
    }
    if (blockIdx.x * RC_THREADS + RC_THREADS <= m) return;           // no divisor in this workgroup (uniform)
    if (p < m || p >= two_m) fe_set_one(v);
    pl_store(tree, S, Lf + t, v);
    lds_tree_invert(tree, Lf, t, [](Fr& ri, const Fr& root) { fe_inverse_safegcd(ri, root); });
    if (p >= m && p < two_m) {
        pl_load(v, tree, S, Lf + t);
        pl_store(zsinv, m, p - m, v);
    }
}

// ---- 2. D_i = ys z(w^(l k)) on a present coset k = i mod m (entry j = i / m of its item), 0 on a missing one ------------------------------
// Blob blockIdx.y: its count l values (count: the items the blob HOLDS, of which the item map may use fewer), its row of n work values, the item map of its index row (item_stride = 0: one row for all) and the
// zdom of its pattern.  BE: the values are 32-byte big-endian integers, decoded on load by the steps of fr_decode_be_to_wire; one >= r counts
// as zero and reports its index in the call, first_value + its place in the group (< 2^28: host_recover.h), through atomicMin on the call's
// one word.
template <bool BE>
__global__ void __launch_bounds__(RC_THREADS)
k_recover_scatter(const uint4* __restrict__ ys, const uint32_t* __restrict__ item_of, uint32_t item_stride, const uint32_t* __restrict__ pattern_of,
                  uint32_t count, uint32_t n, uint32_t m, int log_m, int log_l, const int32_t* __restrict__ zdom, uint4* __restrict__ data,
                  uint32_t first_value, uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * RC_THREADS + threadIdx.x, b = blockIdx.y;
    if (i >= n) return;
    ys += 2 * ((size_t)b * count << log_l);
    item_of += (size_t)b * item_stride;
    zdom += (size_t)pattern_of[b] * NL * m;                          // < patterns of the group by construction (host_recover.h)
    data += 2 * (size_t)b * n;
    const uint32_t k = i & (m - 1), j = i >> log_m, item = item_of[k];
    Fr v;
    fe_set_zero(v);
    if (item != RECOVER_NO_ITEM) {                                   // item < count by construction (host_recover.h)
        Fr z;
        const size_t at = ((size_t)item << log_l) + j;
        if (BE) {
            const uint4 q0 = ys[2 * at], q1 = ys[2 * at + 1];
            const uint32_t raw[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
            uint32_t w32[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) w32[t] = __builtin_bswap32(raw[7 - t]);
            bool below = false;
#pragma unroll
            for (int t = 0; t < 8; ++t) below = w32[t] < FrParams::P32[t] ? true : (w32[t] > FrParams::P32[t] ? false : below);
            if (!below) {
                atomicMin(bad, (first_value + (((uint32_t)b * count + item) << log_l) + j) << 2);
#pragma unroll
                for (int t = 0; t < 8; ++t) w32[t] = 0;
            }
            Fr kin;
            fe_unpack(v, w32);                                       // [0, 2^256): below 5.3 m
#pragma unroll
            for (int t = 0; t < NL; ++t) kin.l[t] = (int32_t)FrParams::K_RAW[t];
            fe_mul(v, v, kin);                                       // 5.3 m * m: v 2^256 in (-m, 2m)
        } else {
            rc_load_words(v, ys, at);                                // < 5.3 m
        }
        pl_load(z, zdom, m, k);                                      // (-m, 2m)
        fe_mul(v, v, z);                                             // |v z| < 5.3 m * 2 m
    }
    rc_store_canon(data, i, v);
}

// ---- 4, 5, 6: the pointwise passes on row blockIdx.y.  MODE 0: entry t times g^t; 1: entry i times zsinv[i mod m] of the blob's pattern;
// 2: entry t times g^-t, and the blob's flag.  MODE 2 writes the first out_len entries of the row to row blockIdx.y of `out`, out_len apart:
// out = data and out_len = n is in place, out_len < n compacts the rows into another buffer for one contiguous download (the entries
// from out_len on are only tested).  BE (MODE 2): the stored entries leave as 32 big-endian bytes; the flag tests the canonical words as before.
template <int MODE, bool BE = false>
__global__ void __launch_bounds__(RC_THREADS)
k_recover_scale(uint4* data, uint32_t n, RcPow gp, const int32_t* __restrict__ zsinv, const uint32_t* __restrict__ pattern_of, uint32_t m,
                uint32_t degree_bound, uint32_t* __restrict__ flag, uint4* out, uint32_t out_len) {
    const uint32_t i = blockIdx.x * RC_THREADS + threadIdx.x, b = blockIdx.y;
    bool nonzero = false;
    if (i < n) {
        Fr v, f;
        rc_load_words(v, data + 2 * (size_t)b * n, i);               // < 5.3 m
        if (MODE == 1) pl_load(f, zsinv + (size_t)pattern_of[b] * NL * m, m, i & (m - 1));
        else rc_gpow(f, gp, i);
        fe_mul(v, v, f);                                             // |v f| < 5.3 m * 2 m
        if (MODE != 2) rc_store_canon(data + 2 * (size_t)b * n, i, v);
        else {
            fe_canon(v);                                             // (-m, 2m) -> canonical: the flag tests the words whether or not they are stored
            if (i < out_len) {
                if (BE) {
                    uint32_t w[8], o[8];
                    fe_pack(w, v);
                    fr_encode_wire_to_be(o, w);                      // words < m, times 32
                    out[2 * ((size_t)b * out_len + i)] = make_uint4(o[0], o[1], o[2], o[3]);
                    out[2 * ((size_t)b * out_len + i) + 1] = make_uint4(o[4], o[5], o[6], o[7]);
                } else {
                    rc_store_words(out + 2 * (size_t)b * out_len, i, v);
                }
            }
            nonzero = i >= degree_bound && !fe_is_literal_zero(v);
        }
    }
    if (MODE == 2) {
        if (__syncthreads_or(nonzero) && threadIdx.x == 0) flag[b] = 1u;   // every writer stores the same word
    }
}

// ---- 7'. evaluation rows leaving as bytes: `total` canonical wire values in place, one lane per value, 2 x uint4 in and out ----------------
__global__ void __launch_bounds__(RC_THREADS)
k_fr_encode_be(uint4* __restrict__ rows, size_t total) {
    const size_t i = (size_t)blockIdx.x * RC_THREADS + threadIdx.x;
    if (i >= total) return;
    const uint4 q0 = rows[2 * i], q1 = rows[2 * i + 1];
    const uint32_t w[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    uint32_t o[8];
    fr_encode_wire_to_be(o, w);                                      // canonical words < m, times 32
    rows[2 * i] = make_uint4(o[0], o[1], o[2], o[3]);
    rows[2 * i + 1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// the factored tables of g^t and g^-t for t < 2^log_n in ctx->rc[2], built on ctx->stream when the context has none that long
static int32_t recover_gpow_tables(kzg_ctx* ctx, int log_n, RcPow* fwd, RcPow* inv) {
    const int have = ctx->rc_gpow_log;
    const int log = std::max(log_n, have);
    const uint32_t hi_len = log > RC_LO_BITS ? 1u << (log - RC_LO_BITS) : 1u;
    const size_t set = (size_t)NL * (RC_LO_LEN + hi_len);            // words of one direction
    if (log_n > have) {
        ctx->rc_gpow_log = -1;
        KZG_HIP_TRY(ctx, ctx->rc[2].reserve(2 * set * 4));
    }
    int32_t* base = ctx->rc[2].as<int32_t>();
    fwd->lo = base; fwd->hi = base + (size_t)NL * RC_LO_LEN; fwd->hi_len = hi_len;
    inv->lo = base + set; inv->hi = base + set + (size_t)NL * RC_LO_LEN; inv->hi_len = hi_len;
    if (log_n > have) {
        for (int d = 0; d < 2; ++d) {
            const RcPow& t = d ? *inv : *fwd;
            hipLaunchKernelGGL(k_recover_gpow_table, dim3(RC_LO_LEN / RC_THREADS), dim3(RC_THREADS), 0, ctx->stream, const_cast<int32_t*>(t.lo), RC_LO_LEN, 1u, d);
            hipLaunchKernelGGL(k_recover_gpow_table, dim3((hi_len + RC_THREADS - 1) / RC_THREADS), dim3(RC_THREADS), 0, ctx->stream, const_cast<int32_t*>(t.hi), hi_len, RC_LO_LEN, d);
        }
        KZG_HIP_TRY(ctx, hipGetLastError());
        ctx->rc_gpow_log = log;                                      // read by later work of the same stream only
    }
    return KZG_OK;
}

// The blobs [b0, b0 + g) of the plan: one launch per stage, the blob as grid.y, the pattern as a grid dimension of the vanishing values.
// `fresh`: upload indices and patterns and compute the vanishing values (false: those of the previous group serve, one index row).
// The values come from the host (words or bytes, staged alike: 32 B each) or lie on the device already; the rows leave as words or as bytes
// (io: RecoverIo, engine.h).  d_bad: the bad word of a call on serialized values, behind the plan's layout in rc[1].
static int32_t recover_run_group(kzg_ctx* ctx, const RecoverBatchPlan& plan, size_t b0, size_t g, bool fresh, const NttTables& tb, const RcPow& gp,
                                 const RcPow& gpi, const RecoverIo& io, uint32_t* d_bad) {
    hipStream_t st = ctx->stream;
    const size_t n = plan.n, l = plan.l, m = plan.m, out_len = plan.out_len;
    const size_t count = plan.value_stride();                        // the items a blob holds where the values lie (plan.count of them are used)
    uint32_t* small = ctx->rc[1].as<uint32_t>();
    int32_t* zdom = ctx->rc[1].as<int32_t>() + plan.w_zdom;
    int32_t* zsinv = ctx->rc[1].as<int32_t>() + plan.w_zsinv;
    uint4* staged = ctx->rc_ntt.data.as<uint4>();                    // the uploaded values now, the transforms' scratch afterwards, compacted rows at the end
    uint4* data = ctx->rc[0].as<uint4>();
    std::vector<uint32_t> stage;                                     // alive until the synchronisation below
    std::vector<uint32_t> flags(g, 0);
    const uint4* values = staged;
    if (io.d_ys) values = io.d_ys + 2 * b0 * count * l;              // resident: read in place
    else KZG_HIP_TRY(ctx, hipMemcpyAsync(staged, static_cast<const uint8_t*>(io.ys) + b0 * count * l * 32, g * count * l * 32, hipMemcpyHostToDevice, st));
    KZG_HIP_TRY(ctx, hipMemsetAsync(small + plan.w_flag, 0, g * 4, st));
    if (fresh) {
        size_t words = 0;
        const size_t P = recover_batch_stage(plan, b0, g, &stage, &words);
        KZG_HIP_TRY(ctx, hipMemcpyAsync(small, stage.data(), words * 4, hipMemcpyHostToDevice, st));
        // vanishing values: 2 m / 256 column groups x `splits` slices of M x P patterns
        const RecoverSplit sp = recover_vanish_split(m, plan.n_missing, P);
        RcVanishArgs va;
        va.missing = small + plan.w_miss; va.n_missing = (uint32_t)plan.n_missing; va.per_split = sp.per_split; va.m = (uint32_t)m; va.log_l = plan.log_l;
        va.tb = tb; va.gp = gp; va.partial = ctx->rc[1].as<int32_t>() + plan.w_part;
        hipLaunchKernelGGL(k_recover_vanish, dim3(sp.xgroups, sp.splits, (unsigned)P), dim3(RC_THREADS), 0, st, va);
        hipLaunchKernelGGL(k_recover_vanish_fold, dim3(sp.xgroups, (unsigned)P), dim3(RC_THREADS), 0, st, va.partial, sp.splits, (uint32_t)m, zdom, zsinv);
    }
    const dim3 ngrid((unsigned)((n + RC_THREADS - 1) / RC_THREADS), (unsigned)g);
    const uint32_t* pattern_of = small + plan.w_pat;
    const uint32_t item_stride = plan.index_rows == 1 ? 0u : (uint32_t)m;
    if (io.ys_be)
        hipLaunchKernelGGL(k_recover_scatter<true>, ngrid, dim3(RC_THREADS), 0, st, values, small + plan.w_item, item_stride, pattern_of, (uint32_t)count, (uint32_t)n,
                           (uint32_t)m, plan.log_m, plan.log_l, zdom, data, (uint32_t)(b0 * count * l), d_bad);
    else
        hipLaunchKernelGGL(k_recover_scatter<false>, ngrid, dim3(RC_THREADS), 0, st, values, small + plan.w_item, item_stride, pattern_of, (uint32_t)count, (uint32_t)n,
                           (uint32_t)m, plan.log_m, plan.log_l, zdom, data, 0u, static_cast<uint32_t*>(nullptr));
    KZG_HIP_TRY(ctx, hipGetLastError());
    int32_t rc = ntt_run_batch(ctx, data, n, g, true, st, &ctx->rc_ntt);     // f Z
    if (rc != KZG_OK) return rc;
    hipLaunchKernelGGL(k_recover_scale<0>, ngrid, dim3(RC_THREADS), 0, st, data, (uint32_t)n, gp, nullptr, nullptr, (uint32_t)m, 0u, nullptr, nullptr, 0u);
    rc = ntt_run_batch(ctx, data, n, g, false, st, &ctx->rc_ntt);            // (f Z)(g w^i)
    if (rc != KZG_OK) return rc;
    hipLaunchKernelGGL(k_recover_scale<1>, ngrid, dim3(RC_THREADS), 0, st, data, (uint32_t)n, gp, zsinv, pattern_of, (uint32_t)m, 0u, nullptr, nullptr, 0u);
    rc = ntt_run_batch(ctx, data, n, g, true, st, &ctx->rc_ntt);             // f(g X)
    if (rc != KZG_OK) return rc;
    // the rows leave from `data` in place, or, shorter than n, compacted into the transforms' scratch (dead after the last transform): one contiguous download
    uint4* rows = out_len < n ? staged : data;
    // coefficient rows are encoded as they are stored; evaluation rows pass through the last transform as words and are encoded behind it
    if (io.out_be && !plan.eval_form)
        hipLaunchKernelGGL((k_recover_scale<2, true>), ngrid, dim3(RC_THREADS), 0, st, data, (uint32_t)n, gpi, nullptr, nullptr, (uint32_t)m, (uint32_t)plan.degree_bound,
                           small + plan.w_flag, rows, (uint32_t)out_len);
    else
        hipLaunchKernelGGL(k_recover_scale<2>, ngrid, dim3(RC_THREADS), 0, st, data, (uint32_t)n, gpi, nullptr, nullptr, (uint32_t)m, (uint32_t)plan.degree_bound,
                           small + plan.w_flag, rows, (uint32_t)out_len);
    KZG_HIP_TRY(ctx, hipGetLastError());
    if (plan.eval_form) {                                            // out_len = n
        rc = ntt_run_batch(ctx, data, n, g, false, st, &ctx->rc_ntt);
        if (rc != KZG_OK) return rc;
        if (io.out_be) {                                             // g n values fit the group's budget: far below 2^32 workgroups
            hipLaunchKernelGGL(k_fr_encode_be, dim3((unsigned)((g * n + RC_THREADS - 1) / RC_THREADS)), dim3(RC_THREADS), 0, st, data, g * n);
            KZG_HIP_TRY(ctx, hipGetLastError());
        }
    }
    uint32_t bad = 0xFFFFFFFFu;                                      // read with the flags at the group's one synchronisation
    if (io.ys_be) KZG_HIP_TRY(ctx, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(static_cast<uint8_t*>(io.out) + b0 * out_len * 32, rows, g * out_len * 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(flags.data(), small + plan.w_flag, g * 4, hipMemcpyDeviceToHost, st));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (bad != 0xFFFFFFFFu) {                                        // the call ends here; this group's flags are not reported
        if (io.bad_word) *io.bad_word = bad;
        return KZG_ERR_DESERIALIZE;
    }
    if (io.consistent)
        for (size_t i = 0; i < g; ++i) io.consistent[b0 + i] = flags[i] ? 0 : 1;
    return KZG_OK;
}

int32_t recover_run_batch(kzg_ctx* ctx, const RecoverBatchPlan& plan, const RecoverIo& io) {
    RoctxRange range(plan.blobs == 1 ? "kzg:recover_from_cosets" : "kzg:recover_from_cosets_batch");
    NttTables tb;
    int32_t rc = ntt_get_tables(ctx, plan.log_n, false, &tb);
    if (rc != KZG_OK) return rc;
    RcPow gp, gpi;
    rc = recover_gpow_tables(ctx, plan.log_n, &gp, &gpi);
    if (rc != KZG_OK) return rc;
    const size_t cap = plan.groups.group;                            // every group works in the buffers of a full one
    KZG_HIP_TRY(ctx, ctx->rc[0].reserve(cap * plan.n * 32));
    KZG_HIP_TRY(ctx, ctx->rc[1].reserve(plan.w_end * 4 + 16));       // + the bad word of a call on serialized values, behind the layout
    KZG_HIP_TRY(ctx, ctx->rc_ntt.data.reserve(cap * plan.n * 32));   // >= the staged values (count l <= n), the transforms' `data`, the compacted rows
    uint32_t* d_bad = ctx->rc[1].as<uint32_t>() + plan.w_end;
    if (io.ys_be) KZG_HIP_TRY(ctx, hipMemsetAsync(d_bad, 0xFF, 4, ctx->stream));
    for (size_t b0 = 0; b0 < plan.blobs; b0 += cap) {
        const size_t g = std::min(cap, plan.blobs - b0);
        // with one index row every group has the same item map, pattern and vanishing values, at the same place
        rc = recover_run_group(ctx, plan, b0, g, b0 == 0 || plan.index_rows != 1, tb, gp, gpi, io, d_bad);
        if (rc != KZG_OK) return rc;
    }
    return KZG_OK;
}

int32_t recover_run(kzg_ctx* ctx, const RecoverPlan& plan, const uint64_t* ys, bool eval_form, uint64_t* out_poly, int32_t* consistent) {
    RecoverIo io;
    io.ys = ys; io.out = out_poly; io.consistent = consistent;
    return recover_run_batch(ctx, recover_batch_of_one(plan, eval_form), io);
}

}  // namespace kzg

#if defined(KZG_DEVICE_BOUND_CHECK)   // the device bound-check variant only (field29.h, `make boundcheck`)
KZG_BOUND_CHECK_EXPORTS(recover)
#endif
