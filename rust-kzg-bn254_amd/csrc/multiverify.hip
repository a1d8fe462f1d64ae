// multiverify.hip — the Fr side of verifying FK20 coset proofs (multiproof.hip makes them; capi_verify.hip kzg_verify_multiproof_batch checks them):
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
//   * l <= 1024 (k_coset_interp): one pass over the input, everything else in LDS.  A workgroup of 256 lanes takes tiles of E = 512
//     values (l <= 512: E / l cosets side by side, 512 at l = 1, 32 at l = 16; one butterfly per lane and stage) or E = 1024 (l = 1024:
//     one coset, two butterflies per lane), tile after tile with stride gridDim: unpack (no product: the values stay in the wire
//     residue class a 2^256, the twiddles are internal Montgomery, as in ntt.hip), bit-reversed fill, log l radix-2 stages on 9 limb
//     planes of E words, then entry t times r_i l^-1 w^(-k_i t) and a lazy sum per lane ACROSS tiles in registers.  At the end the
//     E / l columns of a tile are folded by a tree in LDS: one partial row of l sums per workgroup, and k_coset_sum_rows adds the
//     rows (row groups per column, the same tree) and writes canonical wire words.  At most 1 024 workgroups.
//   * w^(-k t): one product of two entries of the factored inverse tables of the n-point domain (ntt_get_tables: 2^10 + n / 2^10
//     entries), exponent k t mod n in 64 bits.  The stage twiddles w_l^-q = w_n^(-q m) come from the same tables, once per workgroup.
//   * l > 1024 (few, long cosets): one ntt_run per coset in place, then k_coset_twist_sum_global, one lane per column.  Not tuned.
//   * no atomics, no floating point: A_t is an exact field sum, canonical on output, whatever the grid.
// Lazy-reduction bounds are written at each site (the boundcheck build counts violations: tests/test_gpu_multiproof_verify.py).
// Not tried: radix-4 stages (ntt.hip's), a swizzled or padded plane layout (the first stages touch rows 2 b and 2 b + 1 and the fill
// is bit-reversed: 2-way and worse bank conflicts there), wave shuffles for the first six stages, a per-coset w^(-k) power chain in
// place of the table product, more than one tile in flight per workgroup.
// Measured figures: profiles/multiproof_verify.md.
#include "engine.h"
#include "field29.h"

#include <algorithm>

namespace kzg {

struct MvTables { const int32_t* lo; const int32_t* hi; uint32_t lo_len, hi_len; int lo_bits; };

__device__ __forceinline__ void mv_planes_load(Fr& v, const int32_t* planes, uint32_t stride, uint32_t i) {
#pragma unroll
    for (int j = 0; j < NL; ++j) v.l[j] = planes[j * stride + i];
}
__device__ __forceinline__ void mv_planes_store(int32_t* planes, uint32_t stride, uint32_t i, const Fr& v) {
#pragma unroll
    for (int j = 0; j < NL; ++j) planes[j * stride + i] = v.l[j];
}
// w_n^-e (e < n) from the inverse tables of the domain: normalised, in (-m, 2m)
__device__ __forceinline__ void mv_root_pow(Fr& w, const MvTables& t, uint32_t e) {
    mv_planes_load(w, t.lo, t.lo_len, e & (t.lo_len - 1));
    const uint32_t eh = e >> t.lo_bits;
    if (eh != 0) {
        Fr h;
        mv_planes_load(h, t.hi, t.hi_len, eh);
        fe_mul(w, w, h);
    }
}
// the 256-bit words of a wire element as limbs, no product: < 2^256 < 5.3 m, normalised
__device__ __forceinline__ void mv_load_words(Fr& v, const uint4* __restrict__ p) {
    const uint4 lo = p[0], hi = p[1];
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    fe_unpack(v, w);
}
// acc += v with v normalised in (-m, 2m); every 32nd sum is reduced (|acc| < 2 m + 32 * 2 m = 66 m < 169 m), the others normalised
__device__ __forceinline__ void mv_lazy_add(Fr& acc, const Fr& v, bool reduce) {
    fe_add(acc, acc, v);
    if (reduce) fe_reduce(acc); else fe_norm(acc);
}
// x[p] += x[p + span] for span = E / 2 .. width: the E / width column groups of the planes folded into the first; operands normalised
// in (-m, 2m), sums < 4 m reduced to (-0.0001 m, 1.0001 m) again (fe_reduce_small)
__device__ __forceinline__ void mv_fold(int32_t* x, uint32_t E, uint32_t width, uint32_t tid) {
    for (uint32_t span = E >> 1; span >= width; span >>= 1) {
        for (uint32_t p = tid; p < span; p += 256) {
            Fr a, b;
            mv_planes_load(a, x, E, p);
            mv_planes_load(b, x, E, p + span);
            fe_add(a, a, b);
            fe_reduce_small(a);
            mv_planes_store(x, E, p, a);
        }
        __syncthreads();
    }
}

struct MvArgs {
    const uint4* ys;            // count x l wire values
    const uint64_t* ks;         // count coset indices (< n / l, checked by the host)
    const uint4* weights;       // count wire weights
    uint32_t count;
    int log_l, log_n;
    uint32_t tiles;             // ceil(count / (E / l))
    MvTables tb;                // inverse tables of the n-point domain
    int32_t* partial;           // gridDim rows of 9 planes of l words
};

// dynamic LDS: x 9 x E | scale 9 x (E / l) | stage twiddles 9 x max(l / 2, 1) | coset index E / l
template <int EPT>
__global__ void __launch_bounds__(256)
k_coset_interp(MvArgs a) {
    extern __shared__ int32_t mv_lds[];
    constexpr uint32_t E = 256u * EPT;
    const uint32_t tid = threadIdx.x, l = 1u << a.log_l, cpt = E >> a.log_l, half = l >> 1, ntw = half ? half : 1u;
    const uint32_t n_mask = (1u << a.log_n) - 1u;
    int32_t* x = mv_lds;
    int32_t* sc = x + NL * E;
    int32_t* tw = sc + NL * cpt;
    uint32_t* kk = reinterpret_cast<uint32_t*>(tw + NL * ntw);
    for (uint32_t q = tid; q < half; q += 256) {                    // w_l^-q = w_n^(-q m)
        Fr w;
        mv_root_pow(w, a.tb, q << (a.log_n - a.log_l));
        mv_planes_store(tw, ntw, q, w);
    }
    Fr acc[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) fe_set_zero(acc[e]);
    uint32_t pending = 0;
#pragma unroll 1
    for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const uint32_t first = tile * cpt;
        // per coset: r_i / l in internal form (zero past the end), k_i
        for (uint32_t c = tid; c < cpt; c += 256) {
            const uint32_t i = first + c;
            Fr s;
            uint32_t k = 0;
            fe_set_zero(s);
            if (i < a.count) {
                Fr t;
                mv_load_words(t, a.weights + 2 * (size_t)i);
                Fr kin;
#pragma unroll
                for (int j = 0; j < NL; ++j) kin.l[j] = (int32_t)FrParams::K_IN[j];
                fe_mul(s, t, kin);                                   // wire -> internal: (-m, 2m)
                if (a.log_l) {
                    Fr ninv;
#pragma unroll
                    for (int j = 0; j < NL; ++j) ninv.l[j] = (int32_t)FrParams::NINV[a.log_l * NL + j];
                    fe_mul(s, s, ninv);
                }
                k = (uint32_t)a.ks[i];
            }
            mv_planes_store(sc, cpt, c, s);
            kk[c] = k;
        }
        // values: coset c of the tile at [c l, (c + 1) l), entry j at the bit-reversed position
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const uint32_t p = tid + 256u * e, c = p >> a.log_l, j = p & (l - 1), i = first + c;
            Fr v;
            fe_set_zero(v);
            if (i < a.count) mv_load_words(v, a.ys + 2 * (((size_t)i << a.log_l) + j));
            const uint32_t rj = a.log_l ? __brev(j) >> (32 - a.log_l) : 0u;
            mv_planes_store(x, E, (c << a.log_l) + rj, v);
        }
        __syncthreads();
        // log l decimation-in-time stages.  Bounds: inputs < 2^256 < 5.3 m; stage 0 (every twiddle 1) adds and subtracts them: < 10.6 m;
        // from stage 1 on b w is in (-m, 2m), so a value grows by 2 m per stage: < 10.6 m + 9 * 2 m = 28.6 m, and |b w| < 58 m^2 < 169 m^2.
        // Every value is stored normalised.
#pragma unroll 1
        for (int s = 0; s < a.log_l; ++s) {
            const uint32_t h = 1u << s;
#pragma unroll 1
            for (uint32_t bi = tid; bi < E / 2; bi += 256) {
                const uint32_t q = bi & (h - 1), base = ((bi >> s) << (s + 1)) + q;
                Fr u, v, r0, r1;
                mv_planes_load(u, x, E, base);
                mv_planes_load(v, x, E, base + h);
                if (s != 0) {
                    Fr w;
                    mv_planes_load(w, tw, ntw, q << (a.log_l - 1 - s));
                    fe_mul(v, v, w);
                }
                fe_add(r0, u, v);
                fe_sub(r1, u, v);
                fe_norm(r0);
                fe_norm(r1);
                mv_planes_store(x, E, base, r0);
                mv_planes_store(x, E, base + h, r1);
            }
            __syncthreads();
        }
        // entry t of coset c times r_i l^-1 w^(-k_i t), summed per lane across tiles
        const bool reduce = ++pending == 32;
        if (reduce) pending = 0;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const uint32_t p = tid + 256u * e, c = p >> a.log_l, t = p & (l - 1);
            Fr v, s;
            mv_planes_load(v, x, E, p);
            mv_planes_load(s, sc, cpt, c);
            const uint32_t ex = (uint32_t)(((uint64_t)kk[c] * (uint64_t)t) & (uint64_t)n_mask);
            if (ex != 0) {
                Fr w;
                mv_root_pow(w, a.tb, ex);
                fe_mul(s, s, w);
            }
            fe_mul(v, v, s);                                         // |v s| < 28.6 m * 2 m
            mv_lazy_add(acc[e], v, reduce);
        }
        __syncthreads();                                             // the next tile overwrites x, sc, kk
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        fe_reduce(acc[e]);                                           // |acc| < 66 m -> (-m, 2m), normalised
        mv_planes_store(x, E, tid + 256u * e, acc[e]);
    }
    __syncthreads();
    mv_fold(x, E, l, tid);
    int32_t* row = a.partial + (size_t)blockIdx.x * NL * l;
    for (uint32_t t = tid; t < l; t += 256)
#pragma unroll
        for (int j = 0; j < NL; ++j) row[(size_t)j * l + t] = x[j * E + t];
}

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

constexpr size_t MV_LDS_MAX_L = 1024;
constexpr uint32_t MV_MAX_GROUPS = 1024;

// Enqueued on ctx->stream, called under ctx->mu with the arguments checked (capi_verify.hip): d_ys count x l wire values (OVERWRITTEN when
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
    const size_t lds = ((size_t)NL * E + (size_t)NL * cpt + (size_t)NL * std::max<size_t>(l / 2, 1) + cpt) * 4;     // <= 55 KiB
    if (E == 1024) hipLaunchKernelGGL(k_coset_interp<4>, dim3(groups), dim3(256), lds, st, a);
    else hipLaunchKernelGGL(k_coset_interp<2>, dim3(groups), dim3(256), lds, st, a);
    const int log_cb = std::min(log_l, 8);
    hipLaunchKernelGGL(k_coset_sum_rows, dim3((unsigned)(l >> log_cb)), dim3(256), 0, st, a.partial, groups, log_l, log_cb, d_out);
    KZG_HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

}  // namespace kzg

#if defined(KZG_DEVICE_BOUND_CHECK)   // the device bound-check variant only (field29.h, `make boundcheck`)
KZG_BOUND_CHECK_EXPORTS(multiverify)
#endif
