// ntt.hip — radix-2^K Stockham NTT / inverse NTT over BN254 Fr, LDS-tiled (round 2: two passes at 2^20).
//
// Replaces `GeneralEvaluationDomain::<Fr>::new(n).fft(..)` / `.ifft(..)` at
// primitives/src/polynomial.rs:131-135 and :242-246: natural order in and out on the domain
// {w^i}, w = 5^((r-1)/n) (= PRIMITIVE_ROOTS_OF_UNITY[log2 n], primitives/src/consts.rs:22-52); the
// inverse uses w^-1 and scales by n^-1.
//
// Algorithm (decimation in time, Stockham autosort, P = ceil(log n / 10) passes: 10 + 10 at n = 2^20):
//   pass with radix R = 2^K brings the sub-transform length from n_cur/R to n_cur (stride s = N / n_cur):
//     y[u + j * N/R] = sum_j'  w_{n_cur}^(p j') x[q + s (R p + j')] * w_R^(j j'),   u = q + s p
//   A workgroup (512 threads, one per CU, tiles of 2 048 elements: 2^19, 2^20, >= 2^25 -- or 256 threads, two per CU, tiles of 1 024:
//   the other sizes, round 4) owns tiles of C = TILE / R consecutive units u.  Per tile: the R x C
//   elements come from global memory as canonical 256-bit words (runs of C x 32 B), go through the K radix-2 butterfly stages in
//   LDS (9 limb planes, padded rows; radix-4 steps in registers, their multiplies in independent PAIRS: fe_mul2), and leave as
//   256-bit words again.  The inter-pass twiddle w_{n_cur'}^(p' j') of the NEXT pass is applied at the STORE of this pass (the
//   multiply that brings the lazy value back into (-m, 2m) anyway), so later passes load, unpack and go.  Data stay in the wire
//   residue class (a * 2^256) throughout: the transform is linear and the twiddles are in internal Montgomery form.
//   Round 1 ran three passes (7 + 6 + 7) with 36-byte limb planes in between: SQ counters showed its VALU work fully issued
//   (27 of 45 us per pass) and the rest spent in the un-overlapped load and store phases of a single round of tiles.  Here a
//   workgroup walks several tiles and fetches the NEXT tile's words into registers while it computes the current one.
//   Algorithmic traffic: 64 B per element; this implementation moves P x 64 B.
#include "engine.h"
#include "field29.h"
#include "ntt_plan.h"      // the pass policy: constants, NttPassArgs, ntt_plan

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>

namespace kzg {

// The two tile sizes (ntt_plan.h NTT_TILE_LOG_BIG / _SMALL) as the kernel sees them
template <int TILE_LOG> struct NttTile {
    static constexpr int LOG = TILE_LOG;
    static constexpr int TILE = 1 << TILE_LOG;     // elements per workgroup tile
    static constexpr int THREADS = TILE / NTT_EPT;
    // plane length: rows x (C + 1) words in the row-major layout (C >= 16, so at most TILE / 16 rows), C x (R + 32 / C) in the
    // column-major one (ntt_lds_pos) -> TILE + max(TILE / 16, 32) words
    static constexpr int PL = TILE + (TILE / 16 > 32 ? TILE / 16 : 32);
};

// ---- twiddle tables: planes[9][len] of w^(t * step), internal Montgomery form -----------------------
__device__ __forceinline__ void fr_pow_root(Fr& out, int log_n, bool inverse, uint32_t e) {
    // w_{2^log_n}^e by square-and-multiply from the generated root constants
    Fr base;
    const uint32_t* tab = inverse ? FrParams::ROOT_INV : FrParams::ROOT;
#pragma unroll
    for (int j = 0; j < NL; ++j) base.l[j] = (int32_t)tab[log_n * NL + j];
    Fr acc;
    fe_set_one(acc);
    while (e) {
        if (e & 1u) fe_mul(acc, acc, base);
        fe_sqr(base, base);
        e >>= 1;
    }
    out = acc;
}
__global__ void __launch_bounds__(256)
k_ntt_build_table(int32_t* __restrict__ planes, uint32_t len, int log_n, int inverse, uint32_t step) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= len) return;
    Fr w;
    fr_pow_root(w, log_n, inverse != 0, t * step);
#pragma unroll
    for (int j = 0; j < NL; ++j) planes[(size_t)j * len + t] = w.l[j];
}

__device__ __forceinline__ void load_planes(Fr& v, const int32_t* __restrict__ planes, size_t stride, size_t i) {
#pragma unroll
    for (int j = 0; j < NL; ++j) v.l[j] = planes[(size_t)j * stride + i];
}
// w_N^E from the two-level table (one multiply when E >= lo_len)
__device__ __forceinline__ void twiddle(Fr& w, const int32_t* __restrict__ lo, uint32_t lo_len, int lo_bits,
                                        const int32_t* __restrict__ hi, uint32_t hi_len, uint32_t E) {
    load_planes(w, lo, lo_len, E & (lo_len - 1));
    uint32_t eh = E >> lo_bits;
    if (eh != 0) {
        Fr h;
        load_planes(h, hi, hi_len, eh);
        fe_mul(w, w, h);
    }
}

// LDS position of (row i, column uu) of a tile.  C >= 16 columns: row-major with one pad word per row (consecutive lanes =
// consecutive columns = consecutive banks).  C <= 8 (K >= 8, e.g. the 1024 x 2 tiles of a 2^20 transform): a half-wave touches
// 32 / C different rows, so the layout is column-major with a column stride = R + 32 / C (column uu starts 32 / C banks further) and
// the row index is XOR-swizzled, pos = i ^ (((i >> 2) ^ (i >> 6)) & (32 / C - 1)): the rows of one access differ in bits {2..5}
// (first radix-4 step), {0,1,4,5} (second), {0..3} (later steps, final store) or the top bits (bit-reversed fill), and this map is
// injective on each of these sets -- without it the 1024 x 2 tile ran at 70-77 % LDS bank-conflict cycles (SQ_LDS_BANK_CONFLICT).
__device__ __forceinline__ uint32_t ntt_lds_pos(uint32_t i, uint32_t uu, int log_c, int K) {
    if (log_c >= 4) return i * ((1u << log_c) + 1u) + uu;
    const uint32_t spread = 32u >> log_c;                       // rows per half-wave
    const uint32_t cs = (1u << K) + spread;
    return uu * cs + (i ^ (((i >> 2) ^ (i >> 6)) & (spread - 1u)));
}

// inter-pass twiddles of one pass boundary for every element index: tw[idx] = w_N^((p' j') << log_s') as canonical words
__global__ void __launch_bounds__(256)
k_ntt_build_pass_twiddles(uint4* __restrict__ tw, int log_n, int next_K, int next_log_s,
                          const int32_t* __restrict__ tlo, uint32_t lo_len, int lo_bits, const int32_t* __restrict__ thi, uint32_t hi_len);

// global word index of element (uu, j) of tile `tile` on the INPUT side of the pass
__device__ __forceinline__ size_t ntt_in_index(const NttPassArgs& a, int tile_log, uint32_t tile, uint32_t t, uint32_t& uu, uint32_t& j, bool& valid) {
    const int log_c = tile_log - a.K;
    const uint32_t C = 1u << log_c, R = 1u << a.K, s = 1u << a.log_s;
    if (s >= C) { uu = t & (C - 1); j = t >> log_c; }
    else { const uint32_t q = t & (s - 1); j = (t >> a.log_s) & (R - 1); uu = ((t >> (a.log_s + a.K)) << a.log_s) | q; }
    const uint32_t u = (tile << log_c) + uu;
    valid = u < ((1u << a.log_n) >> a.K);
    const uint32_t q = u & (s - 1), p = u >> a.log_s;
    return (size_t)q + ((size_t)(R * p + j) << a.log_s);
}

// KMAX_T: largest radix 2^K this instantiation takes -- its per-workgroup twiddle table holds 2^(KMAX_T - 1) entries (18 KB at 10, 2.3 KB at 7: the
// three-pass plan of round 6, whose workgroups then fit three per CU)
template <int TILE_LOG, int KMAX_T = NTT_KMAX>
__global__ void __launch_bounds__(NttTile<TILE_LOG>::THREADS)
k_ntt_pass(const uint4* __restrict__ in_words, uint4* __restrict__ out_words, NttPassArgs a,
           const int32_t* __restrict__ tlo, uint32_t lo_len, int lo_bits, const int32_t* __restrict__ thi, uint32_t hi_len,
           const uint4* __restrict__ next_tw /* or nullptr: w_N^(E(idx)) of the next pass for every output index, canonical words of the internal form */) {
    constexpr int NTT_TILE_LOG = TILE_LOG, NTT_TILE = NttTile<TILE_LOG>::TILE, NTT_PL = NttTile<TILE_LOG>::PL, NTT_THREADS = NttTile<TILE_LOG>::THREADS;
    __shared__ int32_t lds[NL * NTT_PL];
    constexpr int NTT_TW = 1 << (KMAX_T - 1);
    __shared__ int32_t twl[NL * NTT_TW];
    const int K = a.K, log_n = a.log_n;
    const uint32_t N = 1u << log_n, R = 1u << K;
    const int log_c = NTT_TILE_LOG - K;
    const uint32_t C = 1u << log_c;
    const uint32_t n_units = N >> K;
    const uint32_t tid = threadIdx.x;
    const bool last = a.next_K == 0;
    // a batch of transforms (ntt_run_batch): row blockIdx.y of N consecutive elements in every buffer; the tables are shared
    in_words += (size_t)blockIdx.y << (log_n + 1);
    out_words += (size_t)blockIdx.y << (log_n + 1);

    // per-workgroup local twiddles w_R^t = w_N^(t * N/R), t < R/2 (the same for every tile of the pass)
    for (uint32_t t = tid; t < (R >> 1); t += NTT_THREADS) {
        Fr w;
        twiddle(w, tlo, lo_len, lo_bits, thi, hi_len, t << (log_n - K));
#pragma unroll
        for (int j = 0; j < NL; ++j) twl[j * NTT_TW + t] = w.l[j];
    }
    if (R == 1 && tid == 0) {
        Fr w; fe_set_one(w);
#pragma unroll
        for (int j = 0; j < NL; ++j) twl[j * NTT_TW] = w.l[j];
    }

    // words of the first tile
    uint4 pre[NTT_EPT][2];
    {
        const uint32_t tile = blockIdx.x;
#pragma unroll
        for (int k = 0; k < NTT_EPT; ++k) {
            uint32_t uu, j; bool valid;
            const size_t idx = ntt_in_index(a, NTT_TILE_LOG, tile, tid + k * NTT_THREADS, uu, j, valid);
            if (valid) { pre[k][0] = in_words[2 * idx]; pre[k][1] = in_words[2 * idx + 1]; }
            else { pre[k][0] = make_uint4(0, 0, 0, 0); pre[k][1] = make_uint4(0, 0, 0, 0); }
        }
    }
    for (uint32_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const uint32_t tile_u0 = tile << log_c;
        // ---- registers -> LDS (bit-reversed rows) ----------------------------------------------
#pragma unroll
        for (int k = 0; k < NTT_EPT; ++k) {
            uint32_t uu, j; bool valid;
            (void)ntt_in_index(a, NTT_TILE_LOG, tile, tid + k * NTT_THREADS, uu, j, valid);
            const uint32_t w32[8] = {pre[k][0].x, pre[k][0].y, pre[k][0].z, pre[k][0].w, pre[k][1].x, pre[k][1].y, pre[k][1].z, pre[k][1].w};
            Fr v;
            fe_unpack(v, w32);                          // canonical, or < 3 m from the previous pass: both fine for the lazy stages
            uint32_t jr = K ? (__brev(j) >> (32 - K)) : 0;
            const uint32_t e = ntt_lds_pos(jr, uu, log_c, K);
#pragma unroll
            for (int l = 0; l < NL; ++l) lds[l * NTT_PL + e] = v.l[l];
        }
        __syncthreads();
        // ---- this tile's inter-pass twiddle words (the STORE phase multiplies by them): with the 1 024-element tile they are issued now and are in
        // flight during the butterfly stages; fetched at the store they are a dependent global load in front of every output product.  Same-box A/B
        // (round 6, tools/time_ntt.py, ms per transform early / at the store): 2^12 0.0364 / 0.0386, 2^16 0.0425 / 0.0453, 2^18 0.0528 / 0.0551,
        // 2^21 0.2646 / 0.2788, 2^22 0.5085 / 0.5323 -- but the 2 048-element tile LOSES (2^19 0.0784 / 0.0768, 2^20 0.1390 / 0.1333), so it keeps the late read.
        // Reading them in front of radix-4 step 1 .. 4 of the 2 048-element tile instead: 0.1319-0.1336 ms at 2^20 against 0.1327 at the store -- noise.
        constexpr bool TW_EARLY = TILE_LOG == NTT_TILE_LOG_SMALL && KMAX_T == NTT_KMAX;    // (the three-pass instantiation keeps 145 VGPRs: three waves per SIMD)
        uint4 twpre[NTT_EPT][2];
        auto fetch_tw = [&]() {
#pragma unroll
            for (int k = 0; k < NTT_EPT; ++k) {
                const uint32_t t = tid + k * NTT_THREADS;
                const uint32_t uu = t & (C - 1), j = t >> log_c;
                const uint32_t u = tile_u0 + uu;
                if (u < n_units) {
                    const size_t idx = (size_t)u + ((size_t)j << (log_n - K));
                    twpre[k][0] = next_tw[2 * idx]; twpre[k][1] = next_tw[2 * idx + 1];
                } else { twpre[k][0] = make_uint4(0, 0, 0, 0); twpre[k][1] = make_uint4(0, 0, 0, 0); }
            }
        };
        if (TW_EARLY && !last && next_tw) fetch_tw();
        // ---- prefetch the next tile's words: in flight during the butterfly stages ---------------
        {
            const uint32_t nt = tile + gridDim.x;
            if (nt < a.n_tiles) {
#pragma unroll
                for (int k = 0; k < NTT_EPT; ++k) {
                    uint32_t uu, j; bool valid;
                    const size_t idx = ntt_in_index(a, NTT_TILE_LOG, nt, tid + k * NTT_THREADS, uu, j, valid);
                    if (valid) { pre[k][0] = in_words[2 * idx]; pre[k][1] = in_words[2 * idx + 1]; }
                    else { pre[k][0] = make_uint4(0, 0, 0, 0); pre[k][1] = make_uint4(0, 0, 0, 0); }
                }
            }
        }
        // ---- K DIT stages in LDS: pairs of stages as radix-4 steps in registers, a last radix-2 stage when K is odd ------
        // Radix-4 step over half-sizes h and 2h on rows i0, i0+h, i0+2h, i0+3h (same butterflies and twiddles as two radix-2
        // stages, so the results are identical): one LDS round trip, one barrier and four limb normalisations per four elements.
        uint32_t log_h = 0;
        for (; log_h + 1 < (uint32_t)K; log_h += 2) {
            const uint32_t h = 1u << log_h;
            for (uint32_t gt = tid; gt < (uint32_t)(NTT_TILE / 4); gt += NTT_THREADS) {
                const uint32_t g = gt >> log_c, uu = gt & (C - 1);
                const uint32_t lowb = g & (h - 1);
                const uint32_t i0 = ((g >> log_h) << (log_h + 2)) | lowb;
                const uint32_t e0 = ntt_lds_pos(i0, uu, log_c, K), e1 = ntt_lds_pos(i0 + h, uu, log_c, K),
                               e2 = ntt_lds_pos(i0 + 2 * h, uu, log_c, K), e3 = ntt_lds_pos(i0 + 3 * h, uu, log_c, K);
                const uint32_t t1 = lowb << (K - 1 - log_h);                 // stage h:  w_R^(lowb R / 2h)
                const uint32_t t2 = lowb << (K - 2 - log_h);                 // stage 2h: w_R^(lowb R / 4h), rows i0 / i0+2h
                const uint32_t t3 = (lowb + h) << (K - 2 - log_h);           //           w_R^((lowb+h) R / 4h), rows i0+h / i0+3h
                Fr a0, a1, a2, a3, w, w3;
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    a0.l[l] = lds[l * NTT_PL + e0];
                    a1.l[l] = lds[l * NTT_PL + e1];
                    a2.l[l] = lds[l * NTT_PL + e2];
                    a3.l[l] = lds[l * NTT_PL + e3];
                }
                Fr p, q;
                if (h == 1) { p = a1; q = a3; }                              // first stage: every twiddle is 1
                else {
#pragma unroll
                    for (int l = 0; l < NL; ++l) w.l[l] = twl[l * NTT_TW + t1];
                    fe_mul2(p, a1, w, q, a3, w);
                }
                Fr b0, b1, b2, b3;
                fe_add(b0, a0, p); fe_sub(b1, a0, p);
                fe_add(b2, a2, q); fe_sub(b3, a2, q);
                Fr u, v;
#pragma unroll
                for (int l = 0; l < NL; ++l) { w.l[l] = twl[l * NTT_TW + t2]; w3.l[l] = twl[l * NTT_TW + t3]; }
                fe_mul2(u, b2, w, v, b3, w3);
                Fr c0, c1, c2, c3;
                fe_add(c0, b0, u); fe_norm(c0);
                fe_sub(c2, b0, u); fe_norm(c2);
                fe_add(c1, b1, v); fe_norm(c1);
                fe_sub(c3, b1, v); fe_norm(c3);
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    lds[l * NTT_PL + e0] = c0.l[l];
                    lds[l * NTT_PL + e1] = c1.l[l];
                    lds[l * NTT_PL + e2] = c2.l[l];
                    lds[l * NTT_PL + e3] = c3.l[l];
                }
            }
            __syncthreads();
        }
        if (log_h < (uint32_t)K) {
            const uint32_t h = 1u << log_h;
            for (uint32_t bt = tid; bt < (uint32_t)(NTT_TILE / 2); bt += NTT_THREADS) {
                uint32_t b = bt >> log_c, uu = bt & (C - 1);
                uint32_t lowb = b & (h - 1);
                uint32_t i0 = ((b >> log_h) << (log_h + 1)) | lowb;
                uint32_t e0 = ntt_lds_pos(i0, uu, log_c, K), e1 = ntt_lds_pos(i0 + h, uu, log_c, K);
                uint32_t tw_idx = lowb << (K - 1 - log_h);                 // (b mod h) * R / (2h)
                Fr x0, x, w, t;
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    x0.l[l] = lds[l * NTT_PL + e0];
                    x.l[l] = lds[l * NTT_PL + e1];
                    w.l[l] = twl[l * NTT_TW + tw_idx];
                }
                if (h == 1) t = x;                         // stage 1: every twiddle is w_R^0 = 1
                else fe_mul(t, x, w);
                Fr y0, y1;
                fe_add(y0, x0, t); fe_norm(y0);
                fe_sub(y1, x0, t); fe_norm(y1);
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    lds[l * NTT_PL + e0] = y0.l[l];
                    lds[l * NTT_PL + e1] = y1.l[l];
                }
            }
            __syncthreads();
        }
        // ---- LDS -> global: rows j, C consecutive units each -------------------------------------------------
#pragma unroll
        for (int k = 0; k < NTT_EPT; ++k) {
            const uint32_t t = tid + k * NTT_THREADS;
            const uint32_t uu = t & (C - 1), j = t >> log_c;
            const uint32_t u = tile_u0 + uu;
            if (u >= n_units) continue;
            const size_t idx = (size_t)u + ((size_t)j << (log_n - K));
            const uint32_t e = ntt_lds_pos(j, uu, log_c, K);
            Fr v;
#pragma unroll
            for (int l = 0; l < NL; ++l) v.l[l] = lds[l * NTT_PL + e];
            uint32_t w32[8];
            if (last) {
                if (a.scale_log_n >= 0) {  // a single-pass inverse transform (or no twiddle array): scale by n^-1, which also reduces to (-m, 2m)
                    Fr kk;
#pragma unroll
                    for (int l = 0; l < NL; ++l) kk.l[l] = (int32_t)FrParams::NINV[a.scale_log_n * NL + l];
                    fe_mul(v, v, kk);
                } else {
                    fe_reduce_small(v);    // no factor: ~70 instructions instead of a 206-instruction product by one
                }
                fe_canon(v);
                fe_pack(w32, v);
            } else {
                // the next pass reads x[q' + s' (R' p' + j')] and needs it times w_{n_cur'}^(p' j') = w_N^(p' j' s'): applied here
                const uint32_t tt = (uint32_t)(idx >> a.next_log_s);
                const uint32_t jn = tt & ((1u << a.next_K) - 1), pn = tt >> a.next_K;
                const uint32_t E = (uint32_t)(((unsigned long long)pn * jn) << a.next_log_s) & (N - 1);
                Fr w;
                if (next_tw) {             // one coalesced 32-byte read (same access pattern as the data) instead of a two-level lookup + multiply
                    const uint4 ta = TW_EARLY ? twpre[k][0] : next_tw[2 * idx], tb2 = TW_EARLY ? twpre[k][1] : next_tw[2 * idx + 1];
                    const uint32_t tw32[8] = {ta.x, ta.y, ta.z, ta.w, tb2.x, tb2.y, tb2.z, tb2.w};
                    fe_unpack(w, tw32);
                } else if (E != 0) twiddle(w, tlo, lo_len, lo_bits, thi, hi_len, E);
                else fe_set_one(w);
                fe_mul(v, v, w);           // (-m, 2m)
#pragma unroll
                for (int l = 0; l < NL; ++l) v.l[l] += (int32_t)FrParams::P[l];      // (0, 3m) < 2^256: a non-negative 256-bit word
                fe_norm(v);
                fe_pack(w32, v);
            }
            out_words[2 * idx] = make_uint4(w32[0], w32[1], w32[2], w32[3]);
            out_words[2 * idx + 1] = make_uint4(w32[4], w32[5], w32[6], w32[7]);
        }
        __syncthreads();                   // the tile's rows are read before the next tile overwrites them
    }
}

__global__ void __launch_bounds__(256)
k_ntt_build_pass_twiddles(uint4* __restrict__ tw, int log_n, int next_K, int next_log_s,
                          const int32_t* __restrict__ tlo, uint32_t lo_len, int lo_bits, const int32_t* __restrict__ thi, uint32_t hi_len,
                          int scale_log_n /* >= 0: every entry times (2^scale_log_n)^-1 (the inverse transform's scaling, folded in) */) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t N = 1u << log_n;
    if (idx >= N) return;
    const uint32_t tt = (uint32_t)(idx >> next_log_s);
    const uint32_t jn = tt & ((1u << next_K) - 1), pn = tt >> next_K;
    const uint32_t E = (uint32_t)(((unsigned long long)pn * jn) << next_log_s) & (N - 1);
    Fr w;
    if (E != 0) twiddle(w, tlo, lo_len, lo_bits, thi, hi_len, E);
    else fe_set_one(w);
    if (scale_log_n >= 0) {
        Fr kk;
#pragma unroll
        for (int l = 0; l < NL; ++l) kk.l[l] = (int32_t)FrParams::NINV[scale_log_n * NL + l];
        fe_norm(w);
        fe_mul(w, w, kk);
    }
    fe_canon(w);
    uint32_t o[8];
    fe_pack(o, w);
    tw[2 * idx] = make_uint4(o[0], o[1], o[2], o[3]);
    tw[2 * idx + 1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// ---- host side ------------------------------------------------------------------------------------
struct TableKey { int dev; int log_n; int inverse; bool operator<(const TableKey& o) const { return dev != o.dev ? dev < o.dev : (log_n != o.log_n ? log_n < o.log_n : inverse < o.inverse); } };
static std::map<TableKey, NttTables> g_tables;
static std::mutex g_tables_mu;

int32_t ntt_get_tables(kzg_ctx* ctx, int log_n, bool inverse, NttTables* out) {
    std::lock_guard<std::mutex> lk(g_tables_mu);
    TableKey key{ctx->device, log_n, inverse ? 1 : 0};
    auto it = g_tables.find(key);
    if (it != g_tables.end()) { *out = it->second; return KZG_OK; }
    NttTables t;
    int lo_bits = log_n < NTT_LO_BITS ? log_n : NTT_LO_BITS;
    t.lo_len = 1u << lo_bits;
    t.lo_bits = lo_bits;
    t.hi_len = 1u << (log_n - lo_bits);
    KZG_HIP_TRY(ctx, hipMalloc(&t.lo, (size_t)t.lo_len * NL * 4));
    KZG_HIP_TRY(ctx, hipMalloc(&t.hi, (size_t)t.hi_len * NL * 4));
    hipLaunchKernelGGL(k_ntt_build_table, dim3((t.lo_len + 255) / 256), dim3(256), 0, ctx->stream, t.lo, t.lo_len, log_n, inverse ? 1 : 0, 1u);
    hipLaunchKernelGGL(k_ntt_build_table, dim3((t.hi_len + 255) / 256), dim3(256), 0, ctx->stream, t.hi, t.hi_len, log_n, inverse ? 1 : 0, t.lo_len);
    KZG_HIP_TRY(ctx, hipGetLastError());
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // built once; afterwards read from any stream of the device
    g_tables[key] = t;
    *out = t;
    return KZG_OK;
}

// the inter-pass twiddle of every element as one 32-byte word (ntt_plan.h NTT_FULL_TW_MAX_LOG), kept per (device, log n, direction, boundary, scaled)
struct PassTwKey { int dev, log_n, inverse, next_K, next_log_s, scaled; bool operator<(const PassTwKey& o) const { return std::tie(dev, log_n, inverse, next_K, next_log_s, scaled) < std::tie(o.dev, o.log_n, o.inverse, o.next_K, o.next_log_s, o.scaled); } };
static std::map<PassTwKey, uint4*> g_pass_tw;
static int32_t ntt_get_pass_twiddles(kzg_ctx* ctx, int log_n, bool inverse, int next_K, int next_log_s, const NttTables& tb, int lo_bits, const uint4** out,
                                     bool scaled) {
    std::lock_guard<std::mutex> lk(g_tables_mu);
    PassTwKey key{ctx->device, log_n, inverse ? 1 : 0, next_K, next_log_s, scaled ? 1 : 0};
    auto it = g_pass_tw.find(key);
    if (it != g_pass_tw.end()) { *out = it->second; return KZG_OK; }
    const size_t n = (size_t)1 << log_n;
    uint4* p = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * 32);
    if (e != hipSuccess) { (void)hipGetLastError(); *out = nullptr; return KZG_OK; }     // no memory: the kernel looks the twiddles up itself
    hipLaunchKernelGGL(k_ntt_build_pass_twiddles, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, p, log_n, next_K, next_log_s,
                       tb.lo, tb.lo_len, lo_bits, tb.hi, tb.hi_len, scaled ? log_n : -1);
    KZG_HIP_TRY(ctx, hipGetLastError());
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // built once; afterwards read from any stream of the device
    g_pass_tw[key] = p;
    *out = p;
    return KZG_OK;
}

// the last context of device `dev` is gone: free what the transforms cached for it (twiddle tables, per-element twiddle arrays)
void ntt_release_device_caches(int dev) {
    std::lock_guard<std::mutex> lk(g_tables_mu);
    for (auto it = g_tables.begin(); it != g_tables.end();) {
        if (it->first.dev == dev) { (void)hipFree(it->second.lo); (void)hipFree(it->second.hi); it = g_tables.erase(it); } else ++it;
    }
    for (auto it = g_pass_tw.begin(); it != g_pass_tw.end();) {
        if (it->first.dev == dev) { (void)hipFree(it->second); it = g_pass_tw.erase(it); } else ++it;
    }
}

// one pass of the plan: THE launch of k_ntt_pass, the switch over its instantiations
static void ntt_launch_pass(const NttPlan& plan, int pi, const uint4* src, uint4* dst, const NttTables& tb, int lo_bits, const uint4* next_tw, hipStream_t st, unsigned rows) {
    const NttPass& s = plan.pass[pi];
#define NTT_LAUNCH(...) hipLaunchKernelGGL((k_ntt_pass<__VA_ARGS__>), dim3(s.grid, rows), dim3(plan.threads), 0, st, src, dst, s.args, tb.lo, tb.lo_len, lo_bits, tb.hi, tb.hi_len, next_tw)
    switch (plan.kernel) {
    case NTT_K_SLIM7: NTT_LAUNCH(NTT_TILE_LOG_SMALL, 7); break;
    case NTT_K_SLIM8: NTT_LAUNCH(NTT_TILE_LOG_SMALL, 8); break;
    case NTT_K_SLIM9: NTT_LAUNCH(NTT_TILE_LOG_SMALL, 9); break;
    case NTT_K_SMALL: NTT_LAUNCH(NTT_TILE_LOG_SMALL); break;
    default: NTT_LAUNCH(NTT_TILE_LOG_BIG); break;
    }
#undef NTT_LAUNCH
}
static_assert(NttTile<NTT_TILE_LOG_SMALL>::THREADS == (1 << NTT_TILE_LOG_SMALL) / NTT_EPT && NttTile<NTT_TILE_LOG_BIG>::THREADS == (1 << NTT_TILE_LOG_BIG) / NTT_EPT,
              "NttPlan::threads is the workgroup size k_ntt_pass is bounded to");

// the driver: plan (ntt_plan.h), tables, the reserves from the plan, then its passes.  `rows` transforms of n points, row r at d_data + r n
// elements, as ONE launch per pass (grid.y = the row; 65 535 rows per launch sequence, more in further sequences): the plan is that of one
// transform, its workspaces hold `rows` rows.  ntt_run is rows = 1.
int32_t ntt_run_batch(kzg_ctx* ctx, void* d_data, size_t n, size_t rows, bool inverse, hipStream_t st, NttWorkspace* ws) {
    if (!st) st = ctx->stream;
    if (!ws) ws = &ctx->ntt;
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_NOT_POWER_OF_TWO;
    if (n > ((size_t)1 << NTT_MAX_LOG)) return KZG_ERR_DOMAIN;
    if (n == 1 || rows == 0) return KZG_OK;
    RoctxRange range(inverse ? "kzg:fr_intt" : "kzg:fr_ntt");
    const int log_n = ilog2_ceil(n);
    NttTables tb;
    int32_t rc = ntt_get_tables(ctx, log_n, inverse, &tb);
    if (rc != KZG_OK) return rc;
    const int lo_bits = log_n < NTT_LO_BITS ? log_n : NTT_LO_BITS;
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
    NttPlan plan = ntt_plan(log_n, inverse, cus, opts().ntt_tile_log);
    constexpr size_t ROWS_MAX = 65535;                                       // grid.y of one launch
    const size_t span = std::min(rows, ROWS_MAX);
    if (plan.bytes_data) KZG_HIP_TRY(ctx, ws->data.reserve(plan.bytes_data * span));
    if (plan.bytes_tmp) KZG_HIP_TRY(ctx, ws->tmp.reserve(plan.bytes_tmp * span));
    for (size_t r0 = 0; r0 < rows; r0 += ROWS_MAX) {
        uint4* const bufs[3] = {reinterpret_cast<uint4*>(d_data) + 2 * n * r0, ws->data.as<uint4>(), ws->tmp.as<uint4>()};      // by NttBuf
        for (int pi = 0; pi < plan.n_passes; ++pi) {
            const NttPass& s = plan.pass[pi];
            const uint4* next_tw = nullptr;
            if (s.tw) {
                rc = ntt_get_pass_twiddles(ctx, log_n, inverse, s.args.next_K, s.args.next_log_s, tb, lo_bits, &next_tw, s.tw_scaled);
                if (rc != KZG_OK) return rc;
                if (s.tw_scaled && !next_tw) ntt_plan_fold_missing(plan);
            }
            ntt_launch_pass(plan, pi, bufs[s.src], bufs[s.dst], tb, lo_bits, next_tw, st, (unsigned)std::min(rows - r0, ROWS_MAX));
        }
    }
    KZG_HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

int32_t ntt_run(kzg_ctx* ctx, void* d_data, size_t n, bool inverse, hipStream_t st, NttWorkspace* ws) { return ntt_run_batch(ctx, d_data, n, 1, inverse, st, ws); }

}  // namespace kzg

#if defined(KZG_DEVICE_BOUND_CHECK)   // the device bound-check variant only (field29.h, `make boundcheck`)
#include "field29.h"
KZG_BOUND_CHECK_EXPORTS(ntt)
#endif
