// multiproof.hip — the KZG proofs of EVERY coset of a domain in one call: Feist-Khovratovich, "Fast amortized KZG proofs" (eprint
// 2023/033, "FK20").  The reference opens one point per call (`compute_proof_with_known_z_fr_index`, prover/src/kzg.rs:187-234); n
// such calls are n full proofs, O(n^2).  FK20 computes all n / l coset proofs in O(n log n).
//
// f = f_0 .. f_{n-1} (n a power of two), w the library's primitive n-th root, chunk length l a power of two, 1 <= l <= n / 2, m = n / l.
// Chunk k < m is the coset {w^(k + j m) : j < l} (evaluation indices k, k + m, k + 2m, ...), its vanishing polynomial X^l - w^(k l);
// pi_k = [q_k(tau)]_1, q_k = f / (X^l - w^(k l)).  For l = 1, pi_k is the proof at z = w^k.
//   1. F^(b) = (f_b, f_{l+b}, ..., f_{(m-1)l+b}, 0 x m), b < l                       (length 2m; l Fr NTTs of size 2m)
//   2. S^(b)_t = [tau^((m-2-t) l + b)]_1, t <= m - 2, then the identity up to 2m      (gathered from the SRS)
//   3. H_t = sum_b FFT_2m(F^(b))_t FFT_2m(S^(b))_t, t < 2m                             (k_fk20_lincomb: 2n scalar multiplications)
//   4. h_u = IFFT_2m(H)[u + m - 1], u < m  (h_{m-1} = 0)                               (one inverse G1 FFT; the slice is read in place)
//   5. pi = DFT_m(h) with the m-th root w^l, natural order                            (one forward G1 FFT)
// FFT_2m(S^(b)) depends only on (SRS, n, l): 2n affine points (128 n bytes), cached on the SRS handle (kzg_srs::multiproof).
//
// Design choices (the G1 FFT is g1fft.hip's generic g1_fft_planes: its stage plan, lanes or pairs by the g1_ifft cost model, radix
// 2^K direct stages while n 2^K lanes fit one wave per SIMD, radix-2 butterflies beyond):
//   * the inverse 2m-point and the forward m-point transform are NOT fused: the slice [m - 1, 2m - 1) between them is read in place
//     (pointer offset, stride 2m) by the second transform's first kernel.  Fusing them (a 4-step split of both) was not tried.
//   * the linear combination is one lane per (frequency, term) with GLV scalars, G = min(l, 64) lanes of one wave per frequency folded by
//     a shuffle tree, and for l > 64 up to 32 waves per frequency whose partial sums a second kernel adds; a lane adds l / (64 W) terms
//     one after the other.  l = 1 is a kernel of its own: one scalar multiplication per frequency, no tree.  Lanes rather than pairs:
//     the stage is one multiplication deep like an FFT stage, and the pair form's gain there (0.83 against 1.25 ms) was not measured here.
//   * the Fr side: l NTTs of 2m points as one batched launch per pass (ntt_run_batch: the row is grid.y).
//   * the cache build transforms the l sequences one after the other (gather, forward FFT, affine conversion each).
//
// The encoder (multiproof_encode, kzg_encode_cosets): d coefficients evaluated on n = r d points, deg f < d.  Every quotient has degree
// < d - l, so steps 1-4 run with d in the place of n (m' = d / l, transforms of 2m' points, the cache entry (d, l), d SRS points): fk20_h,
// shared with multiproof_run.  Step 5 alone sees n: pi = DFT_m(h_0 .. h_{m'-1}, 0 x (m - m')), m = n / l, by g1_fft_planes_padded (g1fft.hip;
// plan in host_encode.h: the spread load instead of the first log2 r radix-2 stages, the zeros never read).  The values are one Fr NTT of
// the zero-extended coefficients, written coset-major (k_encode_gather_cosets).
//
// A batch of blobs (multiproof_encode_batch, kzg_encode_cosets_batch): B blobs of one shape, in groups whose workspace fits a byte budget
// (host_encode.h EncodeBatchPlan).  Every kernel of steps 1-5 and of the values takes the blob as grid.y and a distance between
// consecutive blobs' buffers; one blob (grid.y = 1, every distance unused) is the single call.  One lane serves one (blob, frequency,
// term) of the linear combination rather than looping over the blobs with the table point loaded once: the stage is one scalar
// multiplication deep and pure latency while it is under one wave per SIMD, so more lanes cost nothing there while a loop over B blobs
// is B multiplications deep; the table point is 64 bytes against a 127-step chain, and the blobs' reads of it hit the cache.
// Measured figures: README.md ("multi-proofs", "the encoder"), profiles/multiproof.md, profiles/encode.md and profiles/encode_batch.md.
#include "engine.h"
#include "glv.h"
#include "g1_decode.h"          // the steps of fr_decode_be_to_wire on load, fr_encode_wire_to_be on store
#include "host_header_bytes.h"   // g1_encode_be, g2_encode_be: the few header points of a group are compressed on the host

#include <algorithm>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace kzg {

// planes (stride 2m) of S^(b): t <= m - 2 -> SRS point (m - 2 - t) l + b (< n - l), else the identity
__global__ void __launch_bounds__(256)
k_fk20_gather_srs(const uint4* __restrict__ srs_points, uint32_t m, uint32_t l, uint32_t b, int32_t* __restrict__ planes) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, M = 2 * m;
    if (t >= M) return;
    Xyzz v;
    Affine p;
    if (t + 2 <= m && affine_load(p, srs_points + 4 * ((size_t)(m - 2 - t) * l + b))) xyzz_from_affine(v, p, 0);
    else xyzz_set_inf(v);
    xyzz_store(planes, M, t, v);
}

// coefficient rows: F[b][j] = f[j l + b] for j < m, 0 for m <= j < 2m (wire Fr, 32 B each)
__global__ void __launch_bounds__(256)
k_fk20_scatter_coeffs(const uint4* __restrict__ f, uint32_t m, uint32_t l, uint4* __restrict__ F, size_t f_batch /* Fr elements between blobs (grid.y) */) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, M = 2 * m;
    if (i >= M * l) return;
    f += 2 * blockIdx.y * f_batch;
    F += 2 * (size_t)blockIdx.y * M * l;
    const uint32_t b = i / M, j = i - b * M;
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (j < m) { const size_t s = (size_t)j * l + b; lo = f[2 * s]; hi = f[2 * s + 1]; }
    F[2 * (size_t)i] = lo;
    F[2 * (size_t)i + 1] = hi;
}

// l = 1: H_t = Fhat_t Shat_t, one lane per frequency
__global__ void __launch_bounds__(256)
k_fk20_pointwise(const uint4* __restrict__ fhat, const uint4* __restrict__ shat, uint32_t M, int32_t* __restrict__ out, size_t out_batch /* words between blobs (grid.y) */) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M) return;
    fhat += 2 * (size_t)blockIdx.y * M;
    out += blockIdx.y * out_batch;
    Xyzz r;
    glv_term(r, fhat + 2 * (size_t)t, shat + 4 * (size_t)t);
    xyzz_store(out, M, t, r);
}

// l > 1: slot (t, w) = sum of the terms b = (w tpl + i) G + g (g < G lanes, i < tpl) of frequency t; G = 2^log_g <= 64 consecutive lanes of
// one wave per slot, folded by a shuffle tree; slot (t, w) at index t W + w of `out` (stride M W): H itself when W = 1.  Blob grid.y: its l x M
// rows of fhat follow those of the blob before it, its `out` is out_batch words further; every blob reads the same shat.
__global__ void __launch_bounds__(256)
k_fk20_lincomb(const uint4* __restrict__ fhat, const uint4* __restrict__ shat, uint32_t M, int log_g, uint32_t W, uint32_t tpl, int32_t* __restrict__ out, size_t out_batch) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const uint32_t G = 1u << log_g, g = t & (G - 1), slot = t >> log_g;
    fhat += 2 * (size_t)blockIdx.y * (((size_t)W * tpl) << log_g) * M;
    out += blockIdx.y * out_batch;
    const uint32_t o = slot / W, w = slot - o * W;
    const bool active = o < M;                                    // no early return: every lane takes part in the tree
    Xyzz acc;
    xyzz_set_inf(acc);
    if (active) {
#pragma unroll 1
        for (uint32_t i = 0; i < tpl; ++i) {
            const size_t e = (size_t)((w * tpl + i) * G + g) * M + o;   // term b, frequency o of the l x M arrays
            Xyzz term, s;
            glv_term(term, fhat + 2 * e, shat + 4 * e);
            xyzz_add<true>(s, acc, term);
            acc = s;
        }
    }
#pragma unroll 1
    for (int d = 1; d < (int)G; d <<= 1) {
        Xyzz other, r;
        const Fq* sp[4] = {&acc.x, &acc.y, &acc.zz, &acc.zzz};
        Fq* tp[4] = {&other.x, &other.y, &other.zz, &other.zzz};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int q = 0; q < NL; ++q) tp[c]->l[q] = __shfl_down(sp[c]->l[q], d, 64);
        other.inf = __shfl_down((int)acc.inf, d, 64) != 0;
        if ((lane & (2 * d - 1)) == 0) {
            xyzz_add<true>(r, acc, other);
            acc = r;
        }
    }
    if (active && g == 0) xyzz_store(out, (size_t)M * W, slot, acc);
}

// H_t = sum of the W partial sums of frequency t (one lane per frequency)
__global__ void __launch_bounds__(256)
k_fk20_sum_partials(const int32_t* __restrict__ partial, uint32_t M, uint32_t W, int32_t* __restrict__ out, size_t partial_batch, size_t out_batch) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M) return;
    partial += blockIdx.y * partial_batch;
    out += blockIdx.y * out_batch;
    Xyzz acc;
    xyzz_load(acc, partial, (size_t)M * W, (size_t)t * W);
#pragma unroll 1
    for (uint32_t w = 1; w < W; ++w) {
        Xyzz v, s;
        xyzz_load(v, partial, (size_t)M * W, (size_t)t * W + w);
        xyzz_add<true>(s, acc, v);
        acc = s;
    }
    xyzz_store(out, M, t, acc);
}

// out_inf[i] = 1 where the point is the identity
__global__ void __launch_bounds__(256)
k_fk20_inf_flags(const int32_t* __restrict__ planes, uint32_t n, uint8_t* __restrict__ out_inf, size_t planes_batch) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    planes += blockIdx.y * planes_batch;
    out_inf += (size_t)blockIdx.y * n;
    Xyzz v;
    xyzz_load(v, planes, n, i);
    out_inf[i] = v.inf ? 1 : 0;
}

static inline unsigned grid_of(size_t threads) { return (unsigned)((threads + 255) / 256); }

// ---- the cache: FFT_2m(S^(b)) for b < l as l x 2m device-format affine points -------------------------------------------------
static uint4* cached(const kzg_srs* srs, size_t n, size_t l) {
    std::lock_guard<std::mutex> lk(srs->lazy_mu);
    auto it = srs->multiproof.find(std::make_pair(n, l));
    return it == srs->multiproof.end() ? nullptr : it->second;
}

// called under ctx->mu (one builder per context; only the SRS's own context builds); published complete under lazy_mu
int32_t multiproof_cache(kzg_ctx* ctx, kzg_srs* srs, size_t n, size_t l, const uint4** out) {
    if (uint4* c = cached(srs, n, l)) { *out = c; return KZG_OK; }
    const size_t m = n / l, M = 2 * m;
    hipStream_t st = ctx->stream;
    KZG_HIP_TRY(ctx, ctx->mp[2].reserve(M * 36 * 4));
    KZG_HIP_TRY(ctx, ctx->mp[3].reserve(M * 36 * 4));
    KZG_HIP_TRY(ctx, ctx->mp[4].reserve(M * 36 * 4));
    KZG_HIP_TRY(ctx, ctx->mp[5].reserve(M * NL * 4));
    uint4* table = nullptr;
    KZG_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&table), 2 * n * 64));
    int32_t rc = KZG_OK;
    for (size_t b = 0; b < l && rc == KZG_OK; ++b) {
        hipLaunchKernelGGL(k_fk20_gather_srs, dim3(grid_of(M)), dim3(256), 0, st, srs->d_points, (uint32_t)m, (uint32_t)l, (uint32_t)b, ctx->mp[3].as<int32_t>());
        rc = g1_fft_planes(ctx, st, ctx->mp[3].as<int32_t>(), M, M, ctx->mp[2].as<int32_t>(), ctx->mp[4].as<int32_t>(), false, false);
        if (rc == KZG_OK) rc = g1fft_planes_to_affine(ctx, st, ctx->mp[2].as<int32_t>(), M, table + 4 * b * M, false, ctx->mp[5].as<int32_t>());
    }
    if (rc == KZG_OK) {
        hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = set_error(ctx, e, "building the multi-proof cache");
    }
    if (rc != KZG_OK) { (void)hipFree(table); return rc; }
    std::lock_guard<std::mutex> lk(srs->lazy_mu);
    srs->multiproof[std::make_pair(n, l)] = table;
    *out = table;
    return KZG_OK;
}

void multiproof_drop(kzg_srs* srs) {
    std::lock_guard<std::mutex> lk(srs->lazy_mu);
    for (auto& kv : srs->multiproof) (void)hipFree(kv.second);
    srs->multiproof.clear();
}

// ---- the proofs -------------------------------------------------------------------------------------------------------------------
// Steps 1-4 for d coefficients on the device (f), shared by multiproof_run (d = n) and multiproof_encode (d <= n): the l rows F^(b)
// and their NTTs, H = sum_b Fhat^(b) o Shat^(b), the inverse transform of H.  m = d / l, M = 2m; F: l x M wire values; sets.P[0] (M W points),
// P[1], P[2] (M points each or more): plane sets.  *x = the set that holds IFFT_2m(H) (stride M: h is its slice [m - 1, 2m - 1)),
// *y = the plane set that is free again (P[2] stays scratch).  Enqueued on st.
// B blobs (grid.y of every launch): blob b's coefficients at f + b f_batch elements, its rows at F + b l M, its plane sets at
// P[i] + b P_batch[i] words; the l B rows are one batched NTT, the inverse transform's plan is chosen for B (g1fft_plan.h).
struct Fk20Sets { int32_t* P[3]; size_t P_batch[3]; };
static int32_t fk20_h(kzg_ctx* ctx, hipStream_t st, const uint4* shat, const uint4* f, uint4* F, size_t d, size_t l, const Fk20Shape& sh,
                      const Fk20Sets& sets, int* x, int* y, size_t B = 1, size_t f_batch = 0) {
    const size_t m = d / l, M = 2 * m;
    const int log_g = sh.log_g;
    const uint32_t W = sh.W, tpl = sh.tpl;
    const unsigned by = (unsigned)B;
    int32_t* const* P = sets.P;
    const size_t* Pb = sets.P_batch;
    hipLaunchKernelGGL(k_fk20_scatter_coeffs, dim3(grid_of(M * l), by), dim3(256), 0, st, f, (uint32_t)m, (uint32_t)l, F, f_batch);
    int32_t rc = ntt_run_batch(ctx, F, M, l * B, false, st, &ctx->mp_ntt);
    if (rc != KZG_OK) return rc;
    // 2. H = sum_b Fhat^(b) o Shat^(b)
    const int h = W > 1 ? 1 : 0;
    if (l == 1) {
        hipLaunchKernelGGL(k_fk20_pointwise, dim3(grid_of(M), by), dim3(256), 0, st, F, shat, (uint32_t)M, P[h], Pb[h]);
    } else {
        hipLaunchKernelGGL(k_fk20_lincomb, dim3(grid_of((M * W) << log_g), by), dim3(256), 0, st, F, shat, (uint32_t)M, log_g, W, tpl, P[0], Pb[0]);
        if (W > 1) hipLaunchKernelGGL(k_fk20_sum_partials, dim3(grid_of(M), by), dim3(256), 0, st, P[0], (uint32_t)M, W, P[h], Pb[0], Pb[h]);
    }
    KZG_HIP_TRY(ctx, hipGetLastError());
    // 3. h = IFFT_2m(H)[m - 1, 2m - 1): left in place for the next transform to read (offset m - 1, stride 2m)
    const int xi = 1 - h;                                                        // the plane set H is not in
    G1fftBatch gb;
    gb.batch = B; gb.in_batch = Pb[h]; gb.out_batch = Pb[xi]; gb.tmp_batch = Pb[2];
    rc = g1_fft_planes(ctx, st, P[h], M, M, P[xi], P[2], true, true, gb);
    if (rc != KZG_OK) return rc;
    *x = xi;
    *y = h;                                                                      // free again
    return KZG_OK;
}

// 5. m points of planes Y -> wire affine points (identity = zeros) and identity flags in `work` (m x 64 B | m x NL words | m flags), copied out.
// B blobs (plane sets Y_batch words apart): B m points, `work` laid out for B m, one download per output array.
// compressed: out_xy receives 32 gnark-compressed bytes per point (the first half of the same region of `work`), the identity is in the bytes: no flags.
static int32_t fk20_emit(kzg_ctx* ctx, hipStream_t st, const int32_t* Y, size_t m, uint8_t* work, void* out_xy, uint8_t* out_inf, size_t B = 1, size_t Y_batch = 0,
                         bool compressed = false) {
    const size_t pts = B * m;
    uint4* d_aff = reinterpret_cast<uint4*>(work);                               // pts x 64 B
    int32_t* aff_scratch = reinterpret_cast<int32_t*>(work + pts * 64);          // pts x NL words
    uint8_t* d_inf = work + pts * (64 + NL * 4);
    if (compressed) {
        int32_t rc = g1fft_planes_to_affine(ctx, st, Y, m, d_aff, true, aff_scratch, B, Y_batch, true);
        if (rc != KZG_OK) return rc;
        KZG_HIP_TRY(ctx, hipMemcpyAsync(out_xy, d_aff, pts * 32, hipMemcpyDeviceToHost, st));
        return KZG_OK;
    }
    int32_t rc = g1fft_planes_to_affine(ctx, st, Y, m, d_aff, true, aff_scratch, B, Y_batch);
    if (rc != KZG_OK) return rc;
    hipLaunchKernelGGL(k_fk20_inf_flags, dim3(grid_of(m), (unsigned)B), dim3(256), 0, st, Y, (uint32_t)m, d_inf, Y_batch);
    KZG_HIP_TRY(ctx, hipGetLastError());
    KZG_HIP_TRY(ctx, hipMemcpyAsync(out_xy, d_aff, pts * 64, hipMemcpyDeviceToHost, st));
    if (out_inf) KZG_HIP_TRY(ctx, hipMemcpyAsync(out_inf, d_inf, pts, hipMemcpyDeviceToHost, st));
    return KZG_OK;
}

// called under ctx->mu with the arguments checked (capi_srs.hip kzg_compute_multiproofs)
int32_t multiproof_run(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* poly_mont, size_t n, bool eval_form, size_t l, uint64_t* out_xy, uint8_t* out_inf) {
    RoctxRange range("kzg:multiproofs");
    const uint4* shat = nullptr;
    int32_t rc = multiproof_cache(ctx, srs, n, l, &shat);
    if (rc != KZG_OK) return rc;
    const size_t m = n / l, M = 2 * m;
    hipStream_t st = ctx->stream;
    const Fk20Shape sh = fk20_shape(l);                                          // W waves per frequency when l > 64 (<= 32), a lane adding tpl terms
    KZG_HIP_TRY(ctx, ctx->mp[0].reserve(n * 32));
    KZG_HIP_TRY(ctx, ctx->mp[1].reserve(2 * n * 32));
    KZG_HIP_TRY(ctx, ctx->mp[2].reserve(M * sh.W * 36 * 4));
    KZG_HIP_TRY(ctx, ctx->mp[3].reserve(M * 36 * 4));
    KZG_HIP_TRY(ctx, ctx->mp[4].reserve(M * 36 * 4));
    KZG_HIP_TRY(ctx, ctx->mp[5].reserve(m * (64 + 1 + NL * 4)));
    uint4* f = ctx->mp[0].as<uint4>();
    const Fk20Sets sets = {{ctx->mp[2].as<int32_t>(), ctx->mp[3].as<int32_t>(), ctx->mp[4].as<int32_t>()}, {0, 0, 0}};
    // 1. coefficients (eval form: inverse NTT on the device), then steps 1-4
    KZG_HIP_TRY(ctx, hipMemcpyAsync(f, poly_mont, n * 32, hipMemcpyHostToDevice, st));
    if (eval_form) { rc = ntt_run(ctx, f, n, true, st, &ctx->mp_ntt); if (rc != KZG_OK) return rc; }
    int xi = 0, yi = 0;
    rc = fk20_h(ctx, st, shat, f, ctx->mp[1].as<uint4>(), n, l, sh, sets, &xi, &yi);
    if (rc != KZG_OK) return rc;
    int32_t *X = sets.P[xi], *Y = sets.P[yi];
    // 4. pi = DFT_m(h): the slice is read in place (offset m - 1, stride 2m); Y: stride m
    rc = g1_fft_planes(ctx, st, X + (m - 1), M, m, Y, sets.P[2], false, false);
    if (rc != KZG_OK) return rc;
    // 5. one batched affine conversion (wire form, identity = zeros) and the identity flags
    rc = fk20_emit(ctx, st, Y, m, ctx->mp[5].as<uint8_t>(), out_xy, out_inf);
    if (rc != KZG_OK) return rc;
    KZG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return KZG_OK;
}

// ---- the encoder: cosets of values and their proofs for d coefficients on a domain of n = r d points --------------------------------
// ys[k l + j] = evals[k + j m]: the coset-major order of KZG.cosets (wire Fr, 32 B each).  BE: the values (canonical wire words: the
// transform's last pass writes them so) leave as 32 big-endian bytes each, by the steps of fr_encode_wire_to_be, as k_recover_scale<2, true> does.
template <bool BE = false>
__global__ void __launch_bounds__(256)
k_encode_gather_cosets(const uint4* __restrict__ evals, uint32_t n, int log_l, int log_m, uint4* __restrict__ ys) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    evals += 2 * (size_t)blockIdx.y * n;                           // blob grid.y: rows of n elements on both sides
    ys += 2 * (size_t)blockIdx.y * n;
    const uint32_t k = i >> log_l, j = i & ((1u << log_l) - 1);
    const size_t s = (size_t)k + ((size_t)j << log_m);
    if (BE) {
        const uint4 q0 = evals[2 * s], q1 = evals[2 * s + 1];
        const uint32_t w[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
        uint32_t o[8];
        fr_encode_wire_to_be(o, w);                                // canonical words < m, times 32
        ys[2 * (size_t)i] = make_uint4(o[0], o[1], o[2], o[3]);
        ys[2 * (size_t)i + 1] = make_uint4(o[4], o[5], o[6], o[7]);
        return;
    }
    ys[2 * (size_t)i] = evals[2 * s];
    ys[2 * (size_t)i + 1] = evals[2 * s + 1];
}

static_assert(ENCODE_LIMBS == NL && G1FFT_POINT_BYTES == 4 * NL * 4, "host_encode.h sizes the workspaces from these");

// ---- the encoder on a batch of blobs ----------------------------------------------------------------------------------------------------
// f[b fs + i] = src[b d + i] for i < d, zero for d <= i < fs: the compact rows of a group (uploaded, or inverse-NTT'd in place) into the
// rows the value transform extends (blob grid.y)
// BE: the compact rows are the blobs' bytes, 32-byte big-endian integers, decoded on load by the steps of fr_decode_be_to_wire (a byte
// swap, a strict compare with r, one product); one >= r reports atomicMin(bad, (first_value + b d + i) << 2) on the call's one word (the
// call then ends before anything computed from it leaves).  decoded != nullptr: the wire words also go back to the compact row (the
// lane's own element), where the commitments read them.
template <bool BE = false>
__global__ void __launch_bounds__(256)
k_encode_place_coeffs(const uint4* __restrict__ src, uint32_t d, uint32_t fs, uint4* __restrict__ f, uint32_t first_value, uint32_t* __restrict__ bad,
                      uint4* __restrict__ decoded) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= fs) return;
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (i < d) {
        const size_t s = (size_t)blockIdx.y * d + i;
        lo = src[2 * s]; hi = src[2 * s + 1];
        if (BE) {
            const uint32_t raw[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            uint32_t w[8];
            if (!fr_decode_be_to_wire(w, raw)) atomicMin(bad, (first_value + (uint32_t)s) << 2);      // < 2^28 values in a call
            lo = make_uint4(w[0], w[1], w[2], w[3]); hi = make_uint4(w[4], w[5], w[6], w[7]);
            if (decoded) { decoded[2 * s] = lo; decoded[2 * s + 1] = hi; }
        }
    }
    const size_t o = (size_t)blockIdx.y * fs + i;
    f[2 * o] = lo;
    f[2 * o + 1] = hi;
}
// the same decode in place over `total` staged values (compact rows that the next kernel reads as words: f_stride = d, or an inverse
// transform comes first), one lane per value
__global__ void __launch_bounds__(256)
k_encode_decode_be(uint4* __restrict__ rows, uint32_t total, uint32_t first_value, uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint4 q0 = rows[2 * (size_t)i], q1 = rows[2 * (size_t)i + 1];
    const uint32_t raw[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    uint32_t w[8];
    if (!fr_decode_be_to_wire(w, raw)) atomicMin(bad, (first_value + i) << 2);
    rows[2 * (size_t)i] = make_uint4(w[0], w[1], w[2], w[3]);
    rows[2 * (size_t)i + 1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// ---- the serialized form (kzg_encode_cosets_batch_bytes, kzg_disperse_blobs_bytes) ---------------------------------------------------------
// The drivers below take an EncodeBytesIo (engine.h) or none.  With one: the blobs go up as their bytes, into the buffer the words would go to (32 B
// a value either way), and are decoded where the group's first kernel loads them -- k_encode_place_coeffs<true> for coefficient-form blobs whose rows
// are placed (f_stride > d), k_encode_decode_be in place otherwise (f_stride = d, the single blob, or an inverse transform comes first); the value rows
// leave through k_encode_gather_cosets<true>, the proofs through the compressed form of the affine conversion.  The call's bad word stands behind the
// coefficient rows in mp[0].  Once a group's decoded coefficients are complete, encode_bytes_front reads the bad word (a refused value ends the call
// there: nothing computed from it leaves) and commits the rows: commit_batch_device for the commitments, g2_msm_batch_run over both G2 base sets for the
// headers.  Those run on the slots' streams and return wire points (8 / 16 words a blob), which the host compresses: a blob has one G1 and two G2 elements.
// coeffs: g compact rows of d wire values, enqueued on st; b0: the first blob of the group.
static int32_t encode_bytes_front(kzg_ctx* ctx, kzg_srs* srs, hipStream_t st, const EncodeBytesIo& io, const uint32_t* d_bad, const uint4* coeffs, size_t d, size_t b0, size_t g) {
    uint32_t bad = 0xFFFFFFFFu;
    KZG_HIP_TRY(ctx, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(st));                     // (the G1 and G2 launches run on the slots' streams: the rows are complete)
    if (bad != 0xFFFFFFFFu) {
        if (io.bad_word) *io.bad_word = bad;
        return KZG_ERR_DESERIALIZE;
    }
    if (!io.commitments_be) return KZG_OK;
    std::vector<uint64_t> xy(g * 8);
    int32_t rc = commit_batch_device(ctx, srs, coeffs, d, g, xy.data(), nullptr);
    if (rc != KZG_OK) return rc;
    bool ok = true;
    for (size_t i = 0; i < g; ++i) ok = kzg_host::g1_encode_be(xy.data() + 8 * i, io.commitments_be + 32 * (b0 + i)) && ok;
    if (io.g2_points[0]) {
        std::vector<uint64_t> c2(g * 16), p2(g * 16);
        uint64_t* outs[2] = {c2.data(), p2.data()};
        rc = g2_msm_batch_run(ctx, io.g2_points, 2, coeffs, d, g, outs, nullptr);
        if (rc != KZG_OK) return rc;
        for (size_t i = 0; i < g; ++i) {
            ok = kzg_host::g2_encode_be(c2.data() + 16 * i, io.length_commitments_be + 64 * (b0 + i)) && ok;
            ok = kzg_host::g2_encode_be(p2.data() + 16 * i, io.length_proofs_be + 64 * (b0 + i)) && ok;
        }
    }
    if (!ok) { ctx->last_error = "a commitment of the encoder left the device with a coordinate not below p"; return KZG_ERR_DEVICE; }
    return KZG_OK;
}

// called under ctx->mu with the arguments checked and planned (capi_srs.hip kzg_encode_cosets).  The FK20 steps 1-4 see d only (the
// cache entry is (d, l)); step 5 is the m-point transform of h zero-padded (g1_fft_planes_padded); the values are one n-point NTT of the
// zero-extended coefficients.  io: the serialized form, `src` then the bytes of blob `blob` of the call and the outputs that blob's rows.
static int32_t encode_one(kzg_ctx* ctx, kzg_srs* srs, const void* src, bool eval_form, const EncodePlan& plan, void* out_ys, void* out_xy, uint8_t* out_inf,
                          const EncodeBytesIo* io, size_t blob) {
    RoctxRange range("kzg:encode_cosets");
    const size_t d = plan.d, n = plan.n, l = plan.l, m = plan.m, mp = plan.mp, M = plan.M;
    const uint4* shat = nullptr;
    int32_t rc = KZG_OK;
    if (plan.proofs) { rc = multiproof_cache(ctx, srs, d, l, &shat); if (rc != KZG_OK) return rc; }
    hipStream_t st = ctx->stream;
    KZG_HIP_TRY(ctx, ctx->mp[0].reserve(plan.bytes[0] + (io ? 64 : 0)));          // + the bad word of the serialized form
    for (int i = 1; i < 6; ++i) KZG_HIP_TRY(ctx, ctx->mp[i].reserve(plan.bytes[i]));
    uint4* f = ctx->mp[0].as<uint4>();
    uint4* F = ctx->mp[1].as<uint4>();
    // the d coefficients (eval form: inverse NTT of size d on the device)
    KZG_HIP_TRY(ctx, hipMemcpyAsync(f, src, d * 32, hipMemcpyHostToDevice, st));
    uint32_t* d_bad = reinterpret_cast<uint32_t*>(ctx->mp[0].as<uint8_t>() + plan.bytes[0]);
    if (io) {
        KZG_HIP_TRY(ctx, hipMemsetAsync(d_bad, 0xFF, 4, st));
        hipLaunchKernelGGL(k_encode_decode_be, dim3(grid_of(d)), dim3(256), 0, st, f, (uint32_t)d, (uint32_t)(blob * d), d_bad);
        KZG_HIP_TRY(ctx, hipGetLastError());
    }
    if (eval_form) { rc = ntt_run(ctx, f, d, true, st, &ctx->mp_ntt); if (rc != KZG_OK) return rc; }
    if (io) { rc = encode_bytes_front(ctx, srs, st, *io, d_bad, f, d, blob, 1); if (rc != KZG_OK) return rc; }
    if (plan.proofs) {
        const Fk20Sets sets = {{ctx->mp[2].as<int32_t>(), ctx->mp[3].as<int32_t>(), ctx->mp[4].as<int32_t>()}, {0, 0, 0}};
        int32_t* P2 = sets.P[2];
        int xi = 0, yi = 0;
        rc = fk20_h(ctx, st, shat, f, F, d, l, plan.lincomb, sets, &xi, &yi);
        if (rc != KZG_OK) return rc;
        int32_t *X = sets.P[xi], *Y = sets.P[yi];
        // pi = DFT_m(h_0 .. h_{m'-1}, 0 x (m - m')): the slice is read in place (offset m' - 1, stride 2m'), the zeros are never read
        rc = g1_fft_planes_padded(ctx, st, X + (mp - 1), M, mp, m, Y, P2);
        if (rc != KZG_OK) return rc;
        rc = fk20_emit(ctx, st, Y, m, ctx->mp[5].as<uint8_t>(), out_xy, out_inf, 1, 0, io != nullptr);
        if (rc != KZG_OK) return rc;
    }
    if (plan.values) {
        // the evaluations of the zero-extended coefficients, then coset-major into F (free: its last reader, the linear combination, is enqueued)
        if (n > d) KZG_HIP_TRY(ctx, hipMemsetAsync(f + 2 * d, 0, (n - d) * 32, st));
        rc = ntt_run(ctx, f, n, false, st, &ctx->mp_ntt);
        if (rc != KZG_OK) return rc;
        if (io) hipLaunchKernelGGL(k_encode_gather_cosets<true>, dim3(grid_of(n)), dim3(256), 0, st, f, (uint32_t)n, plan.log_l, plan.log_m, F);
        else hipLaunchKernelGGL(k_encode_gather_cosets<false>, dim3(grid_of(n)), dim3(256), 0, st, f, (uint32_t)n, plan.log_l, plan.log_m, F);
        KZG_HIP_TRY(ctx, hipGetLastError());
        KZG_HIP_TRY(ctx, hipMemcpyAsync(out_ys, F, n * 32, hipMemcpyDeviceToHost, st));
    }
    KZG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return KZG_OK;
}
int32_t multiproof_encode(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* poly_mont, bool eval_form, const EncodePlan& plan, uint64_t* out_ys, uint64_t* out_xy, uint8_t* out_inf) {
    return encode_one(ctx, srs, poly_mont, eval_form, plan, out_ys, out_xy, out_inf, nullptr, 0);
}

// called under ctx->mu with the arguments checked and planned (capi_srs.hip kzg_encode_cosets_batch).  Groups of bp.group blobs, one
// after the other on the context's stream with a synchronisation behind each (the workspace is reused; overlapping a group's copies
// with the next one's kernels was not written).  A group of one is encode_one itself.  Inside a group of g blobs the buffers
// are: mp[0] g rows of f_stride coefficients; mp[1] the compact upload (when f_stride > d), then g x l rows of 2m' (FK20), then g rows
// of n coset-major values; mp[2 .. 4] g plane sets each, set_points[i] points apart; mp[5] g m affine points | scratch | flags.
// io: the serialized form.  polys, out_ys and out_xy are then its blobs_be, ys_be and proofs_be: 32 B a value either way, 32 B a proof instead of 64.
static int32_t encode_groups(kzg_ctx* ctx, kzg_srs* srs, const uint8_t* polys, bool eval_form, const EncodeBatchPlan& bp, uint8_t* out_ys, uint8_t* out_xy, uint8_t* out_inf,
                             const EncodeBytesIo* io) {
    const EncodePlan& plan = bp.one;
    const size_t d = plan.d, n = plan.n, l = plan.l, m = plan.m, mp = plan.mp, M = plan.M, fs = bp.f_stride;
    const size_t proof_bytes = io ? 32 : 64;
    if (bp.group == 1) {
        for (size_t b = 0; b < bp.count; ++b) {
            int32_t rc = encode_one(ctx, srs, polys + b * d * 32, eval_form, plan, out_ys ? out_ys + b * n * 32 : nullptr,
                                    out_xy ? out_xy + b * m * proof_bytes : nullptr, out_xy && out_inf ? out_inf + b * m : nullptr, io, b);
            if (rc != KZG_OK) return rc;
        }
        return KZG_OK;
    }
    RoctxRange range("kzg:encode_cosets_batch");
    const uint4* shat = nullptr;
    int32_t rc = KZG_OK;
    if (plan.proofs) { rc = multiproof_cache(ctx, srs, d, l, &shat); if (rc != KZG_OK) return rc; }
    hipStream_t st = ctx->stream;
    KZG_HIP_TRY(ctx, ctx->mp[0].reserve(bp.bytes[0] + (io ? 64 : 0)));            // + the bad word of the serialized form
    for (int i = 1; i < 6; ++i) KZG_HIP_TRY(ctx, ctx->mp[i].reserve(bp.bytes[i]));
    uint4* f = ctx->mp[0].as<uint4>();
    uint4* F = ctx->mp[1].as<uint4>();
    uint32_t* d_bad = reinterpret_cast<uint32_t*>(ctx->mp[0].as<uint8_t>() + bp.bytes[0]);
    if (io) KZG_HIP_TRY(ctx, hipMemsetAsync(d_bad, 0xFF, 4, st));
    Fk20Sets sets;
    for (int i = 0; i < 3; ++i) { sets.P[i] = ctx->mp[2 + i].as<int32_t>(); sets.P_batch[i] = bp.set_points[i] * 4 * NL; }
    for (size_t b0 = 0; b0 < bp.count; b0 += bp.group) {
        const size_t g = std::min(bp.group, bp.count - b0);           // (the last group may be smaller: its transforms are planned for g)
        const unsigned gy = (unsigned)g;
        const uint8_t* src = polys + b0 * d * 32;
        // the coefficients of the group: one upload; eval form: g inverse NTTs of d points, one launch per pass
        uint4* up = fs == d ? f : F;
        KZG_HIP_TRY(ctx, hipMemcpyAsync(up, src, g * d * 32, hipMemcpyHostToDevice, st));
        const bool decode_on_place = io && fs != d && !eval_form;     // else the staged bytes are decoded in place: their next reader takes words
        if (io && !decode_on_place) hipLaunchKernelGGL(k_encode_decode_be, dim3(grid_of(g * d)), dim3(256), 0, st, up, (uint32_t)(g * d), (uint32_t)(b0 * d), d_bad);
        if (eval_form) { rc = ntt_run_batch(ctx, up, d, g, true, st, &ctx->mp_ntt); if (rc != KZG_OK) return rc; }
        if (decode_on_place)
            hipLaunchKernelGGL(k_encode_place_coeffs<true>, dim3(grid_of(fs), gy), dim3(256), 0, st, up, (uint32_t)d, (uint32_t)fs, f, (uint32_t)(b0 * d), d_bad,
                               io->commitments_be ? up : static_cast<uint4*>(nullptr));
        else if (fs != d)
            hipLaunchKernelGGL(k_encode_place_coeffs<false>, dim3(grid_of(fs), gy), dim3(256), 0, st, up, (uint32_t)d, (uint32_t)fs, f, 0u, static_cast<uint32_t*>(nullptr), static_cast<uint4*>(nullptr));
        if (io) {
            KZG_HIP_TRY(ctx, hipGetLastError());
            // the compact rows (where f_stride > d they live in the buffer FK20 overwrites: these reads come first)
            rc = encode_bytes_front(ctx, srs, st, *io, d_bad, up, d, b0, g);
            if (rc != KZG_OK) return rc;
        }
        if (plan.proofs) {
            int xi = 0, yi = 0;
            rc = fk20_h(ctx, st, shat, f, F, d, l, plan.lincomb, sets, &xi, &yi, g, fs);
            if (rc != KZG_OK) return rc;
            G1fftBatch gb;
            gb.batch = g; gb.in_batch = sets.P_batch[xi]; gb.out_batch = sets.P_batch[yi]; gb.tmp_batch = sets.P_batch[2];
            rc = g1_fft_planes_padded(ctx, st, sets.P[xi] + (mp - 1), M, mp, m, sets.P[yi], sets.P[2], gb);
            if (rc != KZG_OK) return rc;
            rc = fk20_emit(ctx, st, sets.P[yi], m, ctx->mp[5].as<uint8_t>(), out_xy + b0 * m * proof_bytes, out_inf ? out_inf + b0 * m : nullptr, g, sets.P_batch[yi], io != nullptr);
            if (rc != KZG_OK) return rc;
        }
        if (plan.values) {
            rc = ntt_run_batch(ctx, f, n, g, false, st, &ctx->mp_ntt);      // rows of n: the coefficients zero-extended (placed above, or n = d)
            if (rc != KZG_OK) return rc;
            if (io) hipLaunchKernelGGL(k_encode_gather_cosets<true>, dim3(grid_of(n), gy), dim3(256), 0, st, f, (uint32_t)n, plan.log_l, plan.log_m, F);
            else hipLaunchKernelGGL(k_encode_gather_cosets<false>, dim3(grid_of(n), gy), dim3(256), 0, st, f, (uint32_t)n, plan.log_l, plan.log_m, F);
            KZG_HIP_TRY(ctx, hipGetLastError());
            KZG_HIP_TRY(ctx, hipMemcpyAsync(out_ys + b0 * n * 32, F, g * n * 32, hipMemcpyDeviceToHost, st));
        }
        KZG_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return KZG_OK;
}
int32_t multiproof_encode_batch(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* polys_mont, bool eval_form, const EncodeBatchPlan& bp, uint64_t* out_ys, uint64_t* out_xy, uint8_t* out_inf) {
    return encode_groups(ctx, srs, reinterpret_cast<const uint8_t*>(polys_mont), eval_form, bp, reinterpret_cast<uint8_t*>(out_ys), reinterpret_cast<uint8_t*>(out_xy), out_inf, nullptr);
}
int32_t multiproof_encode_batch_bytes(kzg_ctx* ctx, kzg_srs* srs, bool eval_form, const EncodeBatchPlan& bp, const EncodeBytesIo& io) {
    return encode_groups(ctx, srs, io.blobs_be, eval_form, bp, io.ys_be, io.proofs_be, nullptr, &io);
}

}  // namespace kzg

#if defined(KZG_DEVICE_BOUND_CHECK)   // the device bound-check variant only (field29.h, `make boundcheck`)
#include "field29.h"
KZG_BOUND_CHECK_EXPORTS(multiproof)
#endif
