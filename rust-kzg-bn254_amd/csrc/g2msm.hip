// g2msm.hip — the G2 multi-scalar multiplication  sum_i s_i Q_i  on the device, and the device side of the G2 SRS handle.
// Replaces `G2Projective::msm(..)` + `.into_affine()` behind the protocol's length commitment and length proof.
//
// Bucket method with signed c-bit windows over the bases as given (no tables):
//   digits + counting sort   the generic mode of the G1 driver, run through msm.hip (msm_sort_generic): entries index | sign << 31
//                            grouped by bucket, and the buckets' offsets -- nothing in them knows the point type
//   k_g2_accumulate          EQUAL SPLIT of the sorted entries over the lanes, checked XYZZ mixed additions of 128-byte affine points
//   k_g2_bucket_fin          lane partials -> bucket sums (heavy buckets by a whole wave)
//   k_g2_red_*               per window sum_k (k + 1) B_k by chunked running sums, left as W wire-format XYZZ values
// The O(W c) Horner doublings and the one inversion run on the host (host_pairing.h).  What a launch does is decided in g2msm_plan.h.
// Many scalar sets over the SAME bases (the blob headers of one call, g2_msm_batch_run) are one bucket problem per group of blobs: one
// sort with in-blob indices, then every kernel once with the base set as grid.y.  A single MSM is the group of one blob.
// Everything here is integer VALU work: no MFMA.
//
// Register budget (profiles/g2msm.md has the compiler's figures): a G2 accumulator is 8 Fq = 72 limb registers, a gathered point 36, a
// Karatsuba product in flight ~60 more.  k_g2_accumulate is compiled for G2_ACC_WAVES = 2 waves per SIMD (256 registers of the unified
// 512-entry file); the latency-bound kernels run one wave per SIMD.
#include "engine.h"
#include "curve_g2.h"
#include "g2msm_plan.h"
#include "host_pairing.h"

#include <cstring>
#include <vector>

namespace kzg {

// -------------------------------------------------------------------------------------------------
// 1. bucket accumulation: equal split of the sorted entries over the lanes
// -------------------------------------------------------------------------------------------------
// Lane t of the nl launched lanes adds the entries [t L, (t + 1) L), L = ceil(E / nl), whatever buckets they belong to: L mixed
// additions per lane whatever the scalars.  Its partial sums go to
//   head[g]  the part of bucket g that STARTS inside the lane's range (every non-empty bucket has exactly one)
//   cont[t]  the part of the bucket that was already open at the lane's first entry (at most one per lane)
// so bucket g = head[g] + sum of cont[t], t in (t1, t2], t1 = offs[g] / L, t2 = (offs[g + 1] - 1) / L  (k_g2_bucket_fin).
__device__ __noinline__ void g2_flush(const G2Xyzz& acc, bool is_cont, int32_t* __restrict__ head, size_t head_stride, uint32_t g,
                                      int32_t* __restrict__ cont, size_t cont_stride, uint32_t t) {
    if (is_cont) g2_store(cont, cont_stride, t, acc);
    else g2_store(head, head_stride, g, acc);
}

// the lane's work: head / cont are those of the lane's base set
__device__ __forceinline__ void g2_accumulate_lane(const uint4* __restrict__ points, const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ offs,
                                                   uint32_t G, int32_t* __restrict__ head, size_t head_stride, int32_t* __restrict__ cont, size_t cont_stride) {
    const uint32_t nl = gridDim.x * blockDim.x;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t E = offs[G];
    if (E == 0) return;
    const uint32_t L = (E + nl - 1) / nl;
    const unsigned long long b64 = (unsigned long long)t * L;
    if (b64 >= E) return;
    const uint32_t begin = (uint32_t)b64;
    const uint32_t end = (b64 + L < E) ? (uint32_t)(b64 + L) : E;
    uint32_t lo = 0, hi = G;                           // invariant: offs[lo] <= begin < offs[hi]; ends at the non-empty bucket that holds `begin`
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (offs[mid] <= begin) lo = mid; else hi = mid;
    }
    uint32_t g = lo, next = offs[g + 1];
    bool is_cont = offs[g] < begin;
    G2Xyzz acc;
    g2_set_inf(acc);
#pragma unroll 1
    for (uint32_t e = begin; e < end; ++e) {
        if (e >= next) {                               // bucket g ends inside this lane's range
            { const G2Xyzz done = acc; g2_flush(done, is_cont, head, head_stride, g, cont, cont_stride, t); }      // (a copy: acc does not escape into the call)
            do { ++g; next = offs[g + 1]; } while (next <= e);      // (e < E = offs[G]: g + 1 <= G)
            is_cont = false;
            g2_set_inf(acc);
        }
        const uint32_t v = sorted[e];
        G2Affine p;
        if (!g2_affine_load(p, points + 8 * (size_t)(v & 0x7FFFFFFFu))) continue;      // identity base
        g2_madd<false>(acc, p, v >> 31);
    }
    { const G2Xyzz done = acc; g2_flush(done, is_cont, head, head_stride, g, cont, cont_stride, t); }
}

// The buckets are those of every blob of the launch (G = blobs W B, entries = in-blob indices), and grid.y = base set.  Every set reads
// the same `sorted` and `offs`; its partial sums go to head + s G and cont + s nl of buffers whose limb planes are nb G and nb nl values
// apart (the strides passed in).
struct G2BaseSets { const uint4* points[2]; };
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(G2_ACC_WAVES, G2_ACC_WAVES)))
k_g2_accumulate(const G2BaseSets bases, const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ offs, uint32_t G,
                int32_t* __restrict__ head, size_t head_stride, int32_t* __restrict__ cont, size_t cont_stride) {
    const uint32_t s = blockIdx.y;
    g2_accumulate_lane(bases.points[s], sorted, offs, G, head + (size_t)s * G, head_stride, cont + (size_t)s * (gridDim.x * blockDim.x), cont_stride);
}

// -------------------------------------------------------------------------------------------------
// 2. lane partials -> bucket sums
// -------------------------------------------------------------------------------------------------
// (g2_shfl: curve_g2.h)
// Bucket g of the G buckets is stored at a transposed position so that the reduction kernels, where lane t walks chunk t
// (buckets t m .. t m + m - 1), read consecutive addresses across lanes.
__device__ __forceinline__ size_t g2_bucket_pos(uint32_t g, uint32_t m, uint32_t n_chunks) { return (size_t)(g % m) * n_chunks + (g / m); }

// partial k of the bucket whose first lane is t1: k == 0 is head[g], k >= 1 is cont[t1 + k]
__device__ __forceinline__ void g2_partial(G2Xyzz& v, uint32_t g, uint32_t t1, uint32_t k, const int32_t* __restrict__ head, size_t head_stride,
                                           const int32_t* __restrict__ cont, size_t cont_stride) {
    if (k == 0) g2_load(v, head, head_stride, g);
    else g2_load(v, cont, cont_stride, t1 + k);
}
// One lane per bucket.  Buckets of up to G2_NP_SERIAL partials are summed by their lane; heavier ones (skewed or equal scalars: few
// distinct digits) one after the other by the whole wave: lanes take partials round-robin, then a six-step shuffle tree.  The order of
// the additions depends on the plan (nl) and the offsets only.
// This kernel and the four of section 3: grid.y = base set s, whose values sit s G (head, bucket), s nl (cont) and s n_chunks (chunk
// arrays) into buffers whose limb planes are nb times as far apart -- the strides passed in.  The windows are those of every blob of the
// launch (G = blobs W B).
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_g2_bucket_fin(const uint32_t* __restrict__ offs, uint32_t G, uint32_t nl, uint32_t m, uint32_t n_chunks,
                const int32_t* __restrict__ head, size_t head_stride, const int32_t* __restrict__ cont, size_t cont_stride,
                int32_t* __restrict__ bucket, size_t bucket_stride) {
    head += (size_t)blockIdx.y * G; cont += (size_t)blockIdx.y * nl; bucket += (size_t)blockIdx.y * G;
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const uint32_t E = offs[G];
    const uint32_t L = (E + nl - 1) / nl;
    uint32_t t1 = 0, np = 0;
    if (g < G && L) {
        const uint32_t o0 = offs[g], o1 = offs[g + 1];
        if (o1 > o0) { t1 = o0 / L; np = 1 + (o1 - 1) / L - t1; }
    }
    G2Xyzz acc;
    g2_set_inf(acc);
    const bool heavy = np > G2_NP_SERIAL;
    if (!heavy) {
#pragma unroll 1
        for (uint32_t k = 0; k < np; ++k) {
            G2Xyzz v;
            g2_partial(v, g, t1, k, head, head_stride, cont, cont_stride);
            g2_add_into(acc, v);
        }
    }
    unsigned long long todo = __ballot(heavy);
    while (todo) {                                     // wave-uniform
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t hg = __shfl(g, src, 64), ht1 = __shfl(t1, src, 64), hnp = __shfl(np, src, 64);
        G2Xyzz part;
        g2_set_inf(part);
#pragma unroll 1
        for (uint32_t k = lane; k < hnp; k += 64) {
            G2Xyzz v;
            g2_partial(v, hg, ht1, k, head, head_stride, cont, cont_stride);
            g2_add_into(part, v);
        }
#pragma unroll 1
        for (int d = 32; d >= 1; d >>= 1) {
            G2Xyzz u;
            g2_shfl(u, part, d, true);
            g2_add_into(part, u);
        }
        G2Xyzz tot;                                    // lane 0 holds the sum
        g2_shfl(tot, part, 0, false);
        if ((int)lane == src) acc = tot;
    }
    if (g < G) g2_store(bucket, bucket_stride, m ? g2_bucket_pos(g, m, n_chunks) : (size_t)g, acc);
}

// -------------------------------------------------------------------------------------------------
// 3. bucket reduction per window: sum_{k=0}^{B-1} (k + 1) bucket[k], chunks of m = B / T buckets, T chunks per window
//    (the scheme of the G1 generic mode, msm_kernels.h section 6, on G2 values)
// -------------------------------------------------------------------------------------------------
// (a) chunk sums S_t
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_g2_red_chunk_sums(const int32_t* __restrict__ bucket, size_t bucket_stride, uint32_t n_chunks, uint32_t m, int32_t* __restrict__ chunkS, size_t chunk_stride) {
    bucket += (size_t)blockIdx.y * n_chunks * m; chunkS += (size_t)blockIdx.y * n_chunks;      // (n_chunks m = G)
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_chunks) return;
    G2Xyzz acc;
    g2_set_inf(acc);
#pragma unroll 1
    for (uint32_t k = 0; k < m; ++k) {
        G2Xyzz v, r;
        g2_load(v, bucket, bucket_stride, (size_t)k * n_chunks + t);
        g2_add<true>(r, acc, v);
        acc = r;
    }
    g2_store(chunkS, chunk_stride, t, acc);
}
// (b) one block per window: inclusive suffix scan of the T chunk sums (Hillis-Steele through global memory): a[w T + t] = sum_{u >= t} S_u
__global__ void __launch_bounds__(G2_RED_T) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_g2_red_suffix_scan(int32_t* __restrict__ a, int32_t* __restrict__ b, size_t stride, uint32_t T) {
    a += (size_t)blockIdx.y * gridDim.x * T; b += (size_t)blockIdx.y * gridDim.x * T;          // (gridDim.x T = n_chunks)
    const uint32_t t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * T;
    int32_t* src = a;
    int32_t* dst = b;
#pragma unroll 1
    for (uint32_t d = 1; d < T; d <<= 1) {
        if (t < T) {
            G2Xyzz v;
            g2_load(v, src, stride, base + t);
            if (t + d < T) {
                G2Xyzz u, r;
                g2_load(u, src, stride, base + t + d);
                g2_add<true>(r, v, u);
                v = r;
            }
            g2_store(dst, stride, base + t, v);
        }
        __syncthreads();
        int32_t* tmp = src; src = dst; dst = tmp;
    }
    if (src != a && t < T) {                           // the result sits in `a`
        G2Xyzz v;
        g2_load(v, src, stride, base + t);
        g2_store(a, stride, base + t, v);
    }
}
// (c) chunk running sums, seeded with the suffix of the later chunks of the window
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_g2_red_chunk_running(const int32_t* __restrict__ bucket, size_t bucket_stride, const int32_t* __restrict__ suffix, size_t chunk_stride,
                       uint32_t n_chunks, uint32_t T, uint32_t m, int32_t* __restrict__ chunkA) {
    bucket += (size_t)blockIdx.y * n_chunks * m; suffix += (size_t)blockIdx.y * n_chunks; chunkA += (size_t)blockIdx.y * n_chunks;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_chunks) return;
    G2Xyzz run, acc;
    if ((t % T) + 1 < T) g2_load(run, suffix, chunk_stride, t + 1);
    else g2_set_inf(run);
    g2_set_inf(acc);
#pragma unroll 1
    for (uint32_t k = m; k-- > 0;) {
        G2Xyzz v;
        g2_load(v, bucket, bucket_stride, (size_t)k * n_chunks + t);
        g2_add_into(run, v);
        g2_add_into(acc, run);
    }
    g2_store(chunkA, chunk_stride, t, acc);
}
// (d) one block per window: tree sum of the T chunk results, left as wire-format XYZZ (64 u32)
__global__ void __launch_bounds__(G2_RED_T) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_g2_red_window_sum(int32_t* __restrict__ a, size_t stride, uint32_t T, uint32_t* __restrict__ out_wire) {
    a += (size_t)blockIdx.y * gridDim.x * T; out_wire += (size_t)blockIdx.y * gridDim.x * G2_WIRE_WORDS;   // (set s: values s n_windows ..)
    const uint32_t t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * T;
#pragma unroll 1
    for (uint32_t d = T >> 1; d >= 1; d >>= 1) {
        if (t < d) {
            G2Xyzz v, u, r;
            g2_load(v, a, stride, base + t);
            g2_load(u, a, stride, base + t + d);
            g2_add<true>(r, v, u);
            g2_store(a, stride, base + t, r);
        }
        __syncthreads();
    }
    if (t == 0) {
        G2Xyzz v;
        g2_load(v, a, stride, base);
        uint32_t w[G2_WIRE_WORDS];
        g2_to_wire(w, v);
        for (int j = 0; j < (int)G2_WIRE_WORDS; ++j) out_wire[(size_t)blockIdx.x * G2_WIRE_WORDS + j] = w[j];
    }
}

// -------------------------------------------------------------------------------------------------
// 4. points: wire <-> device format, on-twist check, powers of tau
// -------------------------------------------------------------------------------------------------
// *bad = the smallest index of a point that is neither the identity nor on the twist (the caller sets it to 0xFFFFFFFF)
__global__ void __launch_bounds__(256)
k_g2_wire_to_device(const uint4* __restrict__ wire, uint4* __restrict__ out, uint32_t n, uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t w[32], o[32];
#pragma unroll
    for (int k = 0; k < 8; ++k) { const uint4 q = wire[8 * (size_t)i + k]; w[4 * k] = q.x; w[4 * k + 1] = q.y; w[4 * k + 2] = q.z; w[4 * k + 3] = q.w; }
    bool on;
    g2_affine_wire_to_device(o, w, &on);
#pragma unroll
    for (int k = 0; k < 8; ++k) out[8 * (size_t)i + k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    if (!on) atomicMin(bad, i);
}
__global__ void __launch_bounds__(256)
k_g2_device_to_wire(const uint4* __restrict__ in, uint4* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t w[32], o[32];
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { const uint4 q = in[8 * (size_t)i + k]; w[4 * k] = q.x; w[4 * k + 1] = q.y; w[4 * k + 2] = q.z; w[4 * k + 3] = q.w; any |= q.x | q.y | q.z | q.w; }
    g2_affine_device_to_wire(o, w);
#pragma unroll
    for (int k = 0; k < 8; ++k) out[8 * (size_t)i + k] = any ? make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]) : make_uint4(0, 0, 0, 0);
}
// out[i] = [k_i] G2 for canonical integers k_i (8 u32 each): double-and-add from the top bit per lane, one Fq2 inversion per point
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_g2_mul_generator(const uint4* __restrict__ scalars_canonical, uint4* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 a = scalars_canonical[2 * (size_t)i], b = scalars_canonical[2 * (size_t)i + 1];
    const uint32_t k[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t gw[32];
    g2_generator_wire(gw);
    G2Affine gen;
    fq2_from_wire(gen.x, gw);
    fq2_from_wire(gen.y, gw + 16);
    fe_canon(gen.x.c0); fe_canon(gen.x.c1); fe_canon(gen.y.c0); fe_canon(gen.y.c1);
    G2Xyzz acc;
    g2_set_inf(acc);
#pragma unroll 1
    for (int bit = 255; bit >= 0; --bit) {
        G2Xyzz d;
        g2_dbl_impl(d, acc);
        acc = d;
        if ((k[bit >> 5] >> (bit & 31)) & 1u) g2_madd<false>(acc, gen, 0);
    }
    uint32_t o[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) o[j] = 0;
    if (!acc.inf) {
        Fq2 x, y;
        g2_to_affine(x, y, acc);
        fq2_pack_canonical(o, x);
        fq2_pack_canonical(o + 16, y);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) out[8 * (size_t)i + q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
}

// -------------------------------------------------------------------------------------------------
// host driver
// -------------------------------------------------------------------------------------------------
namespace H = kzg_host;

// W wire XYZZ window sums (64 u32 each) -> sum_w 2^(c w) S_w as an affine point: one batched inversion for the window sums, Horner in
// Jacobian coordinates (c doublings and one mixed addition per window), one inversion at the end
static H::G2 g2_horner(const uint32_t* wire, int W, int c) {
    std::vector<H::G2> win((size_t)W);
    std::vector<H::Fq2> den((size_t)W), pre((size_t)W);
    H::Fq2 run = {H::FQ_ONE, H::fq_zero()};
    for (int w = 0; w < W; ++w) {
        H::Fq2 q[4];
        for (int k = 0; k < 4; ++k) { memcpy(q[k].c0.l, wire + (size_t)w * G2_WIRE_WORDS + 16 * k, 32); memcpy(q[k].c1.l, wire + (size_t)w * G2_WIRE_WORDS + 16 * k + 8, 32); }
        win[w].inf = H::is_zero(q[2]);
        win[w].x = q[0]; win[w].y = q[1];
        den[w] = win[w].inf ? H::Fq2{H::FQ_ONE, H::fq_zero()} : H::mul(q[2], q[3]);     // ZZ ZZZ
        pre[w] = run;
        run = H::mul(run, den[w]);
        if (!win[w].inf) { win[w].x = H::mul(q[0], q[3]); win[w].y = H::mul(q[1], q[2]); }   // X ZZZ, Y ZZ: over ZZ ZZZ they are X / ZZ, Y / ZZZ
    }
    H::Fq2 iv = H::inv(run);
    for (int w = W - 1; w >= 0; --w) {
        const H::Fq2 di = H::mul(iv, pre[w]);
        iv = H::mul(iv, den[w]);
        if (!win[w].inf) { win[w].x = H::mul(win[w].x, di); win[w].y = H::mul(win[w].y, di); }
    }
    H::G2Jac acc; acc.inf = true; acc.X = {H::fq_zero(), H::fq_zero()}; acc.Y = acc.X; acc.Z = acc.X;
    for (int w = W - 1; w >= 0; --w) {
        for (int k = 0; k < c; ++k) acc = H::g2j_dbl(acc);
        acc = H::g2j_madd(acc, win[w]);
    }
    if (acc.inf) return H::g2_inf();
    const H::Fq2 zi = H::inv(acc.Z), zi2 = H::sqr(zi);
    H::G2 r; r.inf = false;
    r.x = H::mul(acc.X, zi2);
    r.y = H::mul(acc.Y, H::mul(zi2, zi));
    return r;
}

static DeviceBuffer* g2_ws_buffer(MsmWorkspace& ws, int which) {
    DeviceBuffer* const buffers[G2WS_BUFFERS] = {&ws.head, &ws.cont, &ws.bucket, &ws.chunkS, &ws.chunkTmp, &ws.chunkA};      // (the order of G2WsBuffer)
    return buffers[which];
}

// one launch: `blobs` scalar sets (d_scalars: blobs x n, one after the other; n <= G2MSM_MAX_LAUNCH) over nb shared base sets on slot 0's
// workspace and stream, synchronised: results[s * blobs + b] = the sum of blob b over base set s.  The sort's launches and six more,
// whatever blobs and nb.
static int32_t g2_msm_launch(kzg_ctx* ctx, const uint4* const* d_points, uint32_t nb, const uint4* d_scalars, size_t n, uint32_t blobs, H::G2* results) {
    MsmWorkspace& ws = ctx->msm;
    hipStream_t st = ctx->stream;
    const G2Plan p = g2_make_plan(n, nb, blobs, ctx->acc_wave_slots / 3 * G2_ACC_WAVES);
    {
        const char* error = nullptr;
        const int32_t rc = g2_plan_status(p, n, G2_RESULT_CAP, &error);
        if (error) ctx->last_error = error;
        if (rc != KZG_OK) return rc;
    }
    for (int i = 0; i < G2WS_BUFFERS; ++i) KZG_HIP_TRY(ctx, g2_ws_buffer(ws, i)->reserve(p.bytes[i]));
    { const int32_t rc = msm_pinned_out(ctx, ws); if (rc != KZG_OK) return rc; }
    { const int32_t rc = msm_sort_generic(ctx, ws, st, d_scalars, p.sort); if (rc != KZG_OK) return rc; }
    const uint32_t n_chunks = p.n_chunks(), gc = (n_chunks + 255) / 256, n_windows = p.n_windows();
    const size_t hs = (size_t)nb * p.G, cs = (size_t)nb * p.nl, ks = (size_t)nb * n_chunks;     // plane strides: the sets side by side
    G2BaseSets sets{};
    for (uint32_t s = 0; s < nb; ++s) sets.points[s] = d_points[s];
    uint32_t* d_out = reinterpret_cast<uint32_t*>(ws.pinned_out_dev);
    hipLaunchKernelGGL(k_g2_accumulate, dim3(p.nl / 256, nb), dim3(256), 0, st, sets, ws.sorted.as<uint32_t>(), ws.offs.as<uint32_t>(), p.G,
                       ws.head.as<int32_t>(), hs, ws.cont.as<int32_t>(), cs);
    hipLaunchKernelGGL(k_g2_bucket_fin, dim3((p.G + 255) / 256, nb), dim3(256), 0, st, ws.offs.as<uint32_t>(), p.G, p.nl, p.m, n_chunks, ws.head.as<int32_t>(), hs,
                       ws.cont.as<int32_t>(), cs, ws.bucket.as<int32_t>(), hs);
    hipLaunchKernelGGL(k_g2_red_chunk_sums, dim3(gc, nb), dim3(256), 0, st, ws.bucket.as<int32_t>(), hs, n_chunks, p.m, ws.chunkS.as<int32_t>(), ks);
    hipLaunchKernelGGL(k_g2_red_suffix_scan, dim3(n_windows, nb), dim3(p.T), 0, st, ws.chunkS.as<int32_t>(), ws.chunkTmp.as<int32_t>(), ks, p.T);
    hipLaunchKernelGGL(k_g2_red_chunk_running, dim3(gc, nb), dim3(256), 0, st, ws.bucket.as<int32_t>(), hs, ws.chunkS.as<int32_t>(), ks, n_chunks, p.T, p.m,
                       ws.chunkA.as<int32_t>());
    hipLaunchKernelGGL(k_g2_red_window_sum, dim3(n_windows, nb), dim3(p.T), 0, st, ws.chunkA.as<int32_t>(), ks, p.T, d_out);
    KZG_HIP_TRY(ctx, hipGetLastError());
    KZG_HIP_TRY(ctx, hipStreamSynchronize(st));
    // nb * blobs Horner combinations of ~300 dependent host additions each: on the host pool
    const uint32_t* wire = reinterpret_cast<const uint32_t*>(ws.pinned_out);
    const int W = p.W, c = p.c;
    host_parallel_for((size_t)nb * blobs, [&](size_t k) { results[k] = g2_horner(wire + k * (size_t)W * G2_WIRE_WORDS, W, c); });
    return KZG_OK;
}

// `count` scalar sets of n scalars each over nb shared base sets: launches of g2_batch_group blobs; a blob above G2MSM_MAX_LAUNCH pairs
// goes alone, in parts of at most that many pairs whose sums the host adds
int32_t g2_msm_batch_run(kzg_ctx* ctx, const uint4* const* d_points, uint32_t nb, const void* d_scalars, size_t n, size_t count, uint64_t* const* out_g2,
                         uint8_t* const* out_inf) {
    if (nb != 1 && nb != 2) return KZG_ERR_INVALID_ARG;
    const uint4* sc = static_cast<const uint4*>(d_scalars);
    const uint32_t group = n == 0 || n > G2MSM_MAX_LAUNCH ? 1 : g2_batch_group(n, nb, count, ctx->g2_batch_group);      // (>= 1: nb was checked)
    std::vector<H::G2> results((size_t)nb * group, H::g2_inf()), part(nb);                // (n = 0: no launch, every sum the identity)
    for (size_t lo = 0; lo < count; lo += group) {
        const uint32_t blobs = (uint32_t)std::min<size_t>(group, count - lo);
        for (size_t at = 0; at < n; at += G2MSM_MAX_LAUNCH) {       // (one round unless n > G2MSM_MAX_LAUNCH: then blobs = 1)
            const uint4* pts[2] = {d_points[0] + 8 * at, nb == 2 ? d_points[1] + 8 * at : nullptr};
            H::G2* const dst = at ? part.data() : results.data();
            const int32_t rc = g2_msm_launch(ctx, pts, nb, sc + 2 * (lo * n + at), std::min<size_t>(G2MSM_MAX_LAUNCH, n - at), blobs, dst);
            if (rc != KZG_OK) return rc;
            if (at) for (uint32_t s = 0; s < nb; ++s) results[s] = H::g2_add(results[s], part[s]);
        }
        for (uint32_t s = 0; s < nb; ++s)
            for (uint32_t b = 0; b < blobs; ++b) {
                const H::G2& r = results[(size_t)s * blobs + b];
                H::g2_to_wire(r, out_g2[s] + 16 * (lo + b));
                if (out_inf && out_inf[s]) out_inf[s][lo + b] = r.inf ? 1 : 0;
            }
    }
    return KZG_OK;
}

// the single MSM: the batch of one.  out_g2: 16 nb words, out_inf (may be null): nb bytes
int32_t g2_msm_run(kzg_ctx* ctx, const uint4* const* d_points, uint32_t nb, const void* d_scalars, size_t n, uint64_t* out_g2, uint8_t* out_inf) {
    uint64_t* const outs[2] = {out_g2, out_g2 + 16};
    uint8_t* const infs[2] = {out_inf, out_inf ? out_inf + 1 : nullptr};
    return g2_msm_batch_run(ctx, d_points, nb, d_scalars, n, 1, outs, infs);
}

int32_t g2_upload_points(kzg_ctx* ctx, const uint64_t* g2_mont, size_t n, uint4* d_out, int64_t* bad) {
    *bad = -1;
    if (n == 0) return KZG_OK;
    MsmWorkspace& ws = ctx->msm;
    KZG_HIP_TRY(ctx, ws.bases_wire.reserve(n * 128 + 16));
    uint32_t* d_bad = reinterpret_cast<uint32_t*>(ws.bases_wire.as<char>() + n * 128);
    uint32_t h_bad = 0xFFFFFFFFu;
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ws.bases_wire.p, g2_mont, n * 128, hipMemcpyHostToDevice, ctx->stream));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(d_bad, &h_bad, 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_g2_wire_to_device, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ws.bases_wire.as<uint4>(), d_out, (uint32_t)n, d_bad);
    KZG_HIP_TRY(ctx, hipGetLastError());
    KZG_HIP_TRY(ctx, hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (h_bad != 0xFFFFFFFFu) *bad = (int64_t)h_bad;
    return KZG_OK;
}

int32_t g2_generate_points(kzg_ctx* ctx, const uint64_t tau_mont[4], uint64_t first_power, size_t n, uint4* d_out) {
    if (n == 0) return KZG_OK;
    const uint4* d_powers = nullptr;
    { const int32_t rc = fr_powers_canonical(ctx, tau_mont, first_power, n, &d_powers); if (rc != KZG_OK) return rc; }
    hipLaunchKernelGGL(k_g2_mul_generator, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_powers, d_out, (uint32_t)n);
    KZG_HIP_TRY(ctx, hipGetLastError());
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KZG_OK;
}

int32_t g2_download_points(kzg_ctx* ctx, const uint4* d_points, size_t n, uint64_t* out_g2_mont) {
    if (n == 0) return KZG_OK;
    MsmWorkspace& ws = ctx->msm;
    KZG_HIP_TRY(ctx, ws.bases_wire.reserve(n * 128 + 16));
    hipLaunchKernelGGL(k_g2_device_to_wire, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_points, ws.bases_wire.as<uint4>(), (uint32_t)n);
    KZG_HIP_TRY(ctx, hipGetLastError());
    KZG_HIP_TRY(ctx, hipMemcpyAsync(out_g2_mont, ws.bases_wire.p, n * 128, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KZG_OK;
}

}  // namespace kzg

KZG_BOUND_CHECK_EXPORTS(g2msm)
