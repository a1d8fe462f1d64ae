// coset_kernels.h — the tile transform of the coset interpolation, shared by multiverify.hip (ONE aggregated polynomial for a whole
// batch) and multilocate.hip (one polynomial per GROUP of items): wire unpack, bit-reversed fill, radix-2 stages on limb planes in
// LDS, the factored inverse tables for w^(-k t).  What differs between the two is the end of k_coset_interp:
//   SEG = false   entry t times r_i l^-1 w^(-k_i t) is summed per lane ACROSS tiles and the columns of a tile are folded: one partial
//                 row of l sums per workgroup (multiverify.hip k_coset_sum_rows adds the rows);
//   SEG = true    the same weighted, twisted entry is written back per ITEM as a canonical wire word, in place of the value it came
//                 from; nothing is summed here, so no sum can cross a segment boundary (multilocate.hip k_coset_seg_sum adds the rows
//                 of each segment).
// k_coset_interp_mixed, below them, is the ragged form of SEG = false: classes of different (n, l) in one launch, a workgroup per class.
// Device code only; every lazy-reduction bound is written at its site.
#pragma once
#include "engine.h"
#include "field29.h"
#include "host_coset_mixed.h"   // the class descriptor and the limits of the ragged form (pure host header)

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
// v normalised in (-m, 2m) (a product, or a reduced sum) -> its canonical words at p
__device__ __forceinline__ void mv_store_canonical(uint4* p, Fr& v) {
    fe_canon(v);
    uint32_t o[8];
    fe_pack(o, v);
    p[0] = make_uint4(o[0], o[1], o[2], o[3]);
    p[1] = make_uint4(o[4], o[5], o[6], o[7]);
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
    int32_t* partial;           // SEG = false: gridDim rows of 9 planes of l words
    uint4* rows;                // SEG = true: count x l canonical wire words, item order (may be the memory `ys` points to: a tile reads
                                // all of its items' values before it writes any of their rows, and no two tiles share an item)
};

// dynamic LDS: x 9 x E | scale 9 x (E / l) | stage twiddles 9 x max(l / 2, 1) | coset index E / l
template <int EPT, bool SEG = false>
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
    Fr acc[SEG ? 1 : EPT];                                          // (SEG: unused)
#pragma unroll
    for (int e = 0; e < (SEG ? 1 : EPT); ++e) fe_set_zero(acc[e]);
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
        // entry t of coset c times r_i l^-1 w^(-k_i t): summed per lane across tiles, or (SEG) written back as the item's row
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
            fe_mul(v, v, s);                                         // |v s| < 28.6 m * 2 m; the product is normalised, in (-m, 2m)
            if constexpr (SEG) {
                const uint32_t i = first + c;
                if (i < a.count) mv_store_canonical(a.rows + 2 * (((size_t)i << a.log_l) + t), v);
            } else {
                mv_lazy_add(acc[e], v, reduce);
            }
        }
        __syncthreads();                                             // the next tile overwrites x, sc, kk
    }
    if constexpr (!SEG) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            fe_reduce(acc[e]);                                       // |acc| < 66 m -> (-m, 2m), normalised
            mv_planes_store(x, E, tid + 256u * e, acc[e]);
        }
        __syncthreads();
        mv_fold(x, E, l, tid);
        int32_t* row = a.partial + (size_t)blockIdx.x * NL * l;
        for (uint32_t t = tid; t < l; t += 256)
#pragma unroll
            for (int j = 0; j < NL; ++j) row[(size_t)j * l + t] = x[j * E + t];
    }
}

constexpr size_t MV_LDS_MAX_L = 1024;                 // longer cosets: one ntt_run per coset
constexpr uint32_t MV_MAX_GROUPS = 1024;              // workgroups of k_coset_interp
// dynamic LDS of k_coset_interp<E / 256> at chunk length l (<= 55 KiB)
inline size_t mv_interp_lds_bytes(uint32_t E, size_t l) {
    const size_t cpt = E / l;
    return ((size_t)NL * E + (size_t)NL * cpt + (size_t)NL * (l / 2 > 1 ? l / 2 : 1) + cpt) * 4;
}

// ---- the ragged form: classes of different (n, l) in ONE launch (host_coset_mixed.h plans it; multiverify.hip launches it) ------------------
// A workgroup serves exactly ONE class, which it finds through wg_class[blockIdx.x]; it takes that class's tiles with the stride of the
// workgroups the class was given.  l, n, the cosets per tile, the tile count and the LDS carve-up are therefore uniform across the workgroup:
// every __syncthreads() below has the same trip count on all lanes, and the per-lane accumulators keep one meaning across tiles, column
// t = p & (l - 1).  Values, coset indices and weights stay in the caller's item order: slot j of the class is item perm[first + j], whose values
// start at val_off[item].  One table set, that of the largest domain present: w_s = w_max^(n_max / n_s), so an exponent of class s is
// shifted left by log n_max - log n_s before mv_root_pow -- for the stage twiddles and for the twist k t alike (the product k t in 64 bits
// before it is masked, as above).
static_assert(NL == 9, "host_coset_mixed.h sizes the LDS and the partial rows with 9 limb planes");
static_assert(MV_MAX_GROUPS == kzg_host::MIXED_MAX_GROUPS && MV_LDS_MAX_L == kzg_host::MIXED_LDS_MAX_L, "host_coset_mixed.h plans with the limits of this file");
struct MvMixedArgs {
    const uint4* ys;                          // ragged: the items' values one after the other, caller's order
    const uint64_t* ks;                       // count coset indices (< n_s / l_s, checked by the host), caller's order
    const uint4* weights;                     // count wire weights, caller's order
    const uint32_t* perm;                     // the items sorted by class
    const uint32_t* val_off;                  // per item (caller's index): its first value, in elements (total <= 2^28)
    const kzg_host::MixedClassDev* classes;   // per class
    const uint32_t* wg_class;                 // gridDim entries: the class of each workgroup of this launch
    int log_n_max;
    MvTables tb;                              // inverse tables of the n_max-point domain
    int32_t* partial;                         // plane rows: class s, workgroup g of it at row_off + g * 9 * l_s
};

// dynamic LDS, sized for the largest class of the launch and carved per class:
// x 9 x E | scale 9 x (E / l) | stage twiddles 9 x max(l / 2, 1) | coset index E / l | value offset E / l
template <int EPT>
__global__ void __launch_bounds__(256)
k_coset_interp_mixed(MvMixedArgs a) {
    extern __shared__ int32_t mv_lds[];
    constexpr uint32_t E = 256u * EPT;
    const kzg_host::MixedClassDev d = a.classes[a.wg_class[blockIdx.x]];
    const int log_l = (int)d.log_l, log_n = (int)d.log_n, up = a.log_n_max - log_n;
    const uint32_t tid = threadIdx.x, l = 1u << log_l, cpt = E >> log_l, half = l >> 1, ntw = half ? half : 1u;
    const uint32_t n_mask = (1u << log_n) - 1u, wg = blockIdx.x - d.wg_first;
    int32_t* x = mv_lds;
    int32_t* sc = x + NL * E;
    int32_t* tw = sc + NL * cpt;
    uint32_t* kk = reinterpret_cast<uint32_t*>(tw + NL * ntw);
    uint32_t* vo = kk + cpt;
    for (uint32_t q = tid; q < half; q += 256) {                    // w_l^-q = w_n^(-q m) = w_max^(-(q m) 2^up): q 2^(log n_max - log l) < n_max / 2
        Fr w;
        mv_root_pow(w, a.tb, q << (a.log_n_max - log_l));
        mv_planes_store(tw, ntw, q, w);
    }
    Fr acc[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) fe_set_zero(acc[e]);
    uint32_t pending = 0;
#pragma unroll 1
    for (uint32_t tile = wg; tile < d.tiles; tile += d.wg_count) {
        const uint32_t first = tile * cpt;
        // per coset: r_i / l in internal form (zero past the end), k_i, where its values start
        for (uint32_t c = tid; c < cpt; c += 256) {
            const uint32_t j = first + c;
            Fr s;
            uint32_t k = 0, off = kzg_host::MIXED_NO_ITEM;
            fe_set_zero(s);
            if (j < d.count) {
                const uint32_t i = a.perm[d.first + j];
                Fr t;
                mv_load_words(t, a.weights + 2 * (size_t)i);
                Fr kin;
#pragma unroll
                for (int q = 0; q < NL; ++q) kin.l[q] = (int32_t)FrParams::K_IN[q];
                fe_mul(s, t, kin);                                   // wire -> internal: (-m, 2m)
                if (log_l) {
                    Fr ninv;
#pragma unroll
                    for (int q = 0; q < NL; ++q) ninv.l[q] = (int32_t)FrParams::NINV[log_l * NL + q];
                    fe_mul(s, s, ninv);
                }
                k = (uint32_t)a.ks[i];
                off = a.val_off[i];
            }
            mv_planes_store(sc, cpt, c, s);
            kk[c] = k;
            vo[c] = off;
        }
        __syncthreads();                                             // the fill reads vo
        // values: coset c of the tile at [c l, (c + 1) l), entry j at the bit-reversed position
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const uint32_t p = tid + 256u * e, c = p >> log_l, j = p & (l - 1), off = vo[c];
            Fr v;
            fe_set_zero(v);
            if (off != kzg_host::MIXED_NO_ITEM) mv_load_words(v, a.ys + 2 * ((size_t)off + j));
            const uint32_t rj = log_l ? __brev(j) >> (32 - log_l) : 0u;
            mv_planes_store(x, E, (c << log_l) + rj, v);
        }
        __syncthreads();
        // log l decimation-in-time stages, the bounds of k_coset_interp: inputs < 2^256 < 5.3 m; stage 0 (every twiddle 1) adds and subtracts
        // them: < 10.6 m; from stage 1 on b w is in (-m, 2m), so a value grows by 2 m per stage: < 10.6 m + 9 * 2 m = 28.6 m (log l <= 10), and
        // |b w| < 58 m^2 < 169 m^2.  Every value is stored normalised.
#pragma unroll 1
        for (int s = 0; s < log_l; ++s) {
            const uint32_t h = 1u << s;
#pragma unroll 1
            for (uint32_t bi = tid; bi < E / 2; bi += 256) {
                const uint32_t q = bi & (h - 1), base = ((bi >> s) << (s + 1)) + q;
                Fr u, v, r0, r1;
                mv_planes_load(u, x, E, base);
                mv_planes_load(v, x, E, base + h);
                if (s != 0) {
                    Fr w;
                    mv_planes_load(w, tw, ntw, q << (log_l - 1 - s));
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
        // entry t of coset c times r_i l^-1 w_s^(-k_i t), summed per lane across the tiles of this class.  The lazy rule of k_coset_interp: every
        // 32nd sum is reduced (|acc| < 2 m + 32 * 2 m = 66 m < 169 m), the others normalised.
        const bool reduce = ++pending == 32;
        if (reduce) pending = 0;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const uint32_t p = tid + 256u * e, c = p >> log_l, t = p & (l - 1);
            Fr v, s;
            mv_planes_load(v, x, E, p);
            mv_planes_load(s, sc, cpt, c);
            const uint32_t ex = (uint32_t)(((uint64_t)kk[c] * (uint64_t)t) & (uint64_t)n_mask) << up;   // < n_s 2^up = n_max
            if (ex != 0) {
                Fr w;
                mv_root_pow(w, a.tb, ex);
                fe_mul(s, s, w);
            }
            fe_mul(v, v, s);                                         // |v s| < 28.6 m * 2 m; the product is normalised, in (-m, 2m)
            mv_lazy_add(acc[e], v, reduce);
        }
        __syncthreads();                                             // the next tile overwrites x, sc, kk, vo
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        fe_reduce(acc[e]);                                           // |acc| < 66 m -> (-m, 2m), normalised
        mv_planes_store(x, E, tid + 256u * e, acc[e]);
    }
    __syncthreads();
    mv_fold(x, E, l, tid);
    int32_t* row = a.partial + d.row_off + (size_t)wg * NL * l;
    for (uint32_t t = tid; t < l; t += 256)
#pragma unroll
        for (int j = 0; j < NL; ++j) row[(size_t)j * l + t] = x[j * E + t];
}

}  // namespace kzg
