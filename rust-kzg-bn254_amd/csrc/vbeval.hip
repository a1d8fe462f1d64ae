// vbeval.hip -- the front end of batch verification: all n barycentric evaluations y_i = p_i(z_i) of verify_blob_kzg_proof_batch in two
// launches (k_vb_prep, k_vb_eval), driven in three steps by capi_verify.hip (vb_evaluate_setup / _enqueue / _finish; VbBlob and VB_MAX_LOG
// are engine.h's).  It works in slot 0's buffers; the blobs it does not cover go through the single-polynomial path of poly.hip.
#include "poly_common.h"
#include "fe_invert.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace kzg {

// verifier/src/batch.rs:16-69 -> primitives/src/helpers.rs:613-662 evaluates y_i = p_i(z_i) blob after blob (n_i inversions each).
// Here blob i (2^log_n <= 2^VB_MAX_LOG evaluations, read straight from its big-endian bytes) is one workgroup:
//   k_vb_prep   one LANE per blob: z^n by squarings and the ONE inversion of the blob, 1 / (z^n - 1) = 1 / prod_j (z - w^j) (Fermat)
//   k_vb_eval   one WORKGROUP per blob: lane t owns the denominators d_j = z - w^j, j = t + k Lf; a product tree over the lanes
//               in LDS, seeded at the root with the inverse from k_vb_prep and walked down (lds_tree_invert), leaves every lane the
//               inverse of its own product; Montgomery's trick inside the lane ; then sum_j f_j w^j / (z - w^j) and
//               y = (z^n - 1) / n times that sum (helpers.rs:507-532).
// z on the domain (1 - z^n == 0; the early return of helpers.rs:497-504) and blobs beyond 2^VB_MAX_LOG elements are flagged and evaluated by
// the single-polynomial path (proof_run) on the host's request.
constexpr int VB_THREADS = 512;         // 8 waves: two per SIMD, 256 VGPRs each (the asm products keep inputs and outputs apart)
struct VbPrep { int32_t z[NL]; int32_t znm1[NL]; int32_t tinv[NL]; uint32_t fallback; };

__global__ void __launch_bounds__(64)
k_vb_prep(const uint4* __restrict__ zs_wire, const VbBlob* __restrict__ meta, uint32_t nb, VbPrep* __restrict__ prep) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const int log_n = (int)meta[i].log_n;
    Fr z, zn, one, den;
    wire_load(z, zs_wire, i);
    zn = z;
    for (int a = 0; a < log_n; ++a) fe_sqr(zn, zn);
    fe_set_one(one);
    fe_sub(den, zn, one);
    fe_reduce(den);                                        // z^n - 1 in (-m, 2m)
    Fr dc = den;
    fe_canon(dc);
    VbPrep& o = prep[i];
    o.fallback = (fe_is_literal_zero(dc) || log_n > VB_MAX_LOG) ? 1u : 0u;
    fe_canon(z);
#pragma unroll
    for (int j = 0; j < NL; ++j) { o.z[j] = z.l[j]; o.znm1[j] = den.l[j]; }
    if (o.fallback) return;
    // 1 / den by division steps (fe_invert.h, round 4; a^(r-2) before: 380 dependent products on a lone lane)
    Fr acc;
    fe_inverse_safegcd(acc, den);
#pragma unroll
    for (int j = 0; j < NL; ++j) o.tinv[j] = acc.l[j];
}

// raw big-endian chunk j of a packed blob as a plain integer < 2^256 in limbs (zero beyond the blob's elements)
__device__ __forceinline__ void vb_load_raw(Fr& x, const uint8_t* __restrict__ base, uint32_t j, uint32_t n_elems) {
    uint32_t w32[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (j < n_elems) be_chunk_load(w32, base + (size_t)j * 32);
    fe_unpack(x, w32);
}

// lane t of a blob's workgroup: its M denominators, their product into the tree leaf (phase 1), and after the tree walk the M
// barycentric terms (phase 2).  M = n / Lf in {1, 2, 4, 8}: a template parameter so that d[] / pre[] stay in registers.
template <int M>
struct VbLane {
    Fr d[M], pre[M];
    __device__ __forceinline__ void denominators(Fr& p, const Fr& z, const NttTables& tb, uint32_t t, uint32_t Lf, int sh) {
#pragma unroll
        for (int k = 0; k < M; ++k) {
            Fr w;
            domain_elem(w, tb, (t + (uint32_t)k * Lf) << sh);
            fe_canon(w);
            fe_sub(d[k], z, w);                            // canonical - canonical: limbs within +-2^29, |d| < m
            if (k == 0) p = d[0];
            else { pre[k] = p; fe_mul(p, p, d[k]); }
        }
    }
    __device__ __forceinline__ void terms(Fr& sum, Fr inv_all, const NttTables& tb, const uint8_t* __restrict__ base, uint32_t n_elems, uint32_t t, uint32_t Lf, int sh) {
#pragma unroll
        for (int k = M - 1; k >= 0; --k) {
            Fr inv;
            if (k > 0) { fe_mul(inv, inv_all, pre[k]); fe_mul(inv_all, inv_all, d[k]); }
            else inv = inv_all;
            const uint32_t jdx = t + (uint32_t)k * Lf;
            Fr x, w, term;
            vb_load_raw(x, base, jdx, n_elems);
            domain_elem(w, tb, jdx << sh);
            fe_mul(term, x, w);                            // plain integer x internal form = plain residue f_j w^j
            fe_mul(term, term, inv);
            fe_add(sum, sum, term);
            if (M > 4 && (k & 1) == 0) fe_norm(sum);       // at most four unnormalised 29-bit limbs fit an int32: keep the running sum normalised
        }
        fe_norm(sum);                                      // <= 8 terms of (-m, 2m)
        fe_reduce(sum);
    }
};

template <int M>
__device__ __forceinline__ void vb_eval_body(int32_t* __restrict__ tree, const uint8_t* __restrict__ bytes, const VbBlob& b, const VbPrep& pr,
                                             const NttTables& tb, uint4* __restrict__ ys_wire) {
    const int log_n = (int)b.log_n;
    const uint32_t n = 1u << log_n, Lf = n / (uint32_t)M;
    const uint32_t t = threadIdx.x, n_elems = (b.len + 31) / 32;
    const int sh = VB_MAX_LOG - log_n;                     // w_n^j = w_4096^(j << sh)
    Fr z;
#pragma unroll
    for (int j = 0; j < NL; ++j) z.l[j] = pr.z[j];
    VbLane<M> lane;
    if (t < Lf) {
        Fr p;
        lane.denominators(p, z, tb, t, Lf, sh);
        pl_store(tree, 2 * Lf, Lf + t, p);
    }
    lds_tree_invert(tree, Lf, t, [&](Fr& ri, const Fr&) {   // the root's inverse is k_vb_prep's: 1 / prod_j (z - w^j) = 1 / (z^n - 1)
#pragma unroll
        for (int j = 0; j < NL; ++j) ri.l[j] = pr.tinv[j];
    });
    Fr sum;
    fe_set_zero(sum);
    if (t < Lf) {
        Fr inv_all;
        pl_load(inv_all, tree, 2 * Lf, Lf + t);
        lane.terms(sum, inv_all, tb, bytes + b.off, n_elems, t, Lf, sh);
    }
    __syncthreads();                                       // the tree is dead: its planes carry the block sum
    int level = 0;
    for (uint32_t dd = VB_THREADS / 2; dd >= 1; dd >>= 1, ++level) {
#pragma unroll
        for (int j = 0; j < NL; ++j) tree[j * VB_THREADS + t] = sum.l[j];
        __syncthreads();
        if (t < dd) {
            Fr u;
#pragma unroll
            for (int j = 0; j < NL; ++j) u.l[j] = tree[j * VB_THREADS + t + dd];
            fe_add(sum, sum, u);
            fe_norm(sum);
            if (level % 4 == 3) fe_reduce(sum);            // 16 terms of (-m, 2m) since the last reduction
        }
        __syncthreads();
    }
    if (t != 0) return;
    fe_reduce(sum);
    Fr y, znm1, ninv, kraw;
#pragma unroll
    for (int j = 0; j < NL; ++j) { znm1.l[j] = pr.znm1[j]; ninv.l[j] = (int32_t)FrParams::NINV[log_n * NL + j]; kraw.l[j] = (int32_t)FrParams::K_RAW[j]; }
    fe_mul(y, sum, znm1);
    fe_mul(y, y, ninv);                                    // helpers.rs:529-532; y is a PLAIN residue here (the raw f_j carried no Montgomery factor)
    fe_mul(y, y, kraw);                                    // -> wire form y 2^256
    fe_canon(y);
    uint32_t o[8];
    fe_pack(o, y);
    ys_wire[2 * (size_t)blockIdx.x] = make_uint4(o[0], o[1], o[2], o[3]);
    ys_wire[2 * (size_t)blockIdx.x + 1] = make_uint4(o[4], o[5], o[6], o[7]);
}

__global__ void __launch_bounds__(VB_THREADS)
k_vb_eval(const uint8_t* __restrict__ bytes, const VbBlob* __restrict__ meta, const VbPrep* __restrict__ prep, NttTables tb /* 2^VB_MAX_LOG domain */,
          uint4* __restrict__ ys_wire) {
    extern __shared__ int32_t tree[];                      // NL planes of 2 Lf nodes (heap order: root 1, leaves Lf + t)
    const VbBlob b = meta[blockIdx.x];
    const VbPrep& pr = prep[blockIdx.x];
    if (pr.fallback) return;                               // uniform across the workgroup
    const uint32_t n = 1u << b.log_n;
    if (n <= (uint32_t)VB_THREADS) vb_eval_body<1>(tree, bytes, b, pr, tb, ys_wire);
    else if (n == 2u * VB_THREADS) vb_eval_body<2>(tree, bytes, b, pr, tb, ys_wire);
    else if (n == 4u * VB_THREADS) vb_eval_body<4>(tree, bytes, b, pr, tb, ys_wire);
    else vb_eval_body<8>(tree, bytes, b, pr, tb, ys_wire);
}

// ---- host -----------------------------------------------------------------------------------------------------
// Batched y_i = p_i(z_i) for `nb` blobs whose bytes sit packed in PINNED host memory `packed` (blob i at meta[i].off, 32-byte aligned,
// zero-filled up to the next 32-byte chunk) with the challenges zs (wire).  Three steps so that the caller can overlap the uploads with
// the hashing of later blobs:
//   vb_evaluate_setup(ctx, packed_len, nb)                     buffers, the 4096-point domain table, kernel attribute
//   vb_evaluate_enqueue(ctx, packed, meta, b0, b1, zs)         blobs [b0, b1): their bytes, challenges and descriptors go up and the two
//                                                              kernels are enqueued on the context's stream; returns at once; may be called
//                                                              from any host thread, chunks in any order (they touch disjoint ranges)
//   vb_evaluate_finish(ctx, nb, ys_out, fallback_out)          waits; ys_out = nb wire elements; fallback_out[i] != 0 marks the blobs this
//                                                              path does not cover (z on the domain, more than 2^VB_MAX_LOG elements)
// Slot 0's buffers and stream.
int32_t vb_evaluate_setup(kzg_ctx* ctx, size_t packed_len, size_t nb) {
    PolySet& set = ctx->poly[0];
    NttTables tb;
    int32_t rc = ntt_get_tables(ctx, VB_MAX_LOG, false, &tb);
    if (rc != KZG_OK) return rc;
    KZG_HIP_TRY(ctx, set.c.reserve(packed_len + 64));
    KZG_HIP_TRY(ctx, set.a.reserve(nb * 32 * 2 + 64));                                 // zs | ys
    KZG_HIP_TRY(ctx, set.b.reserve(nb * (sizeof(VbBlob) + sizeof(VbPrep)) + 64));
    KZG_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_vb_eval), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(NL * 2 * VB_THREADS * 4)));
    KZG_HIP_TRY(ctx, hipMemsetAsync(set.a.as<uint4>() + 2 * nb, 0, nb * 32, ctx->stream));
    // slot 1's stream carries the blob bytes: created HERE, on the calling thread under ctx->mu -- vb_evaluate_enqueue runs on the
    // caller's worker threads, which must not create context state (two chunks finishing together raced on stream_x[0])
    hipStream_t st_copy = nullptr;
    return msm_slot_stream(ctx, 1, &st_copy);
}
// `small_pinned`: pinned staging of at least nb x 48 bytes for the chunk's challenges and descriptors (a copy from pageable memory would
// make this call wait for everything queued on the stream before it)
int32_t vb_evaluate_enqueue(kzg_ctx* ctx, const uint8_t* packed, const VbBlob* meta, size_t nb, size_t b0, size_t b1, const uint64_t* zs,
                            uint8_t* small_pinned) {
    if (b1 <= b0) return KZG_OK;
    // worker threads of the caller's pool: errors travel in the return code only (ctx->last_error belongs to the thread holding ctx->mu)
    hipEvent_t up = nullptr;
#define VB_TRY(expr) do { if ((expr) != hipSuccess) { (void)hipGetLastError(); if (up) (void)hipEventDestroy(up); return KZG_ERR_DEVICE; } } while (0)
    VB_TRY(hipSetDevice(ctx->device));
    PolySet& set = ctx->poly[0];
    hipStream_t st = ctx->stream, st_copy = ctx->stream_x[0] ? ctx->stream_x[0] : ctx->stream;   // slot 1's stream exists since vb_evaluate_setup
    // the blob bytes go up on a second stream (slot 1's): k_vb_prep is one inversion deep (~0.2 ms on a few lone waves, whatever the
    // chunk size) and needs the challenges only, so it runs while the chunk's bytes are still on the bus; k_vb_eval waits for them
    NttTables tb;
    int32_t rc = ntt_get_tables(ctx, VB_MAX_LOG, false, &tb);                          // cached by vb_evaluate_setup: a look-up
    if (rc != KZG_OK) return rc;
    uint4* d_zs = set.a.as<uint4>();
    uint4* d_ys = d_zs + 2 * nb;
    VbBlob* d_meta = set.b.as<VbBlob>();
    VbPrep* d_prep = reinterpret_cast<VbPrep*>(d_meta + nb);
    uint32_t max_log = 0;
    size_t lo = SIZE_MAX, hi = 0;
    for (size_t i = b0; i < b1; ++i) {
        if (meta[i].log_n > (uint32_t)VB_MAX_LOG) continue;
        max_log = std::max(max_log, meta[i].log_n);
        lo = std::min<size_t>(lo, meta[i].off);
        hi = std::max<size_t>(hi, meta[i].off + ((size_t)meta[i].len + 31) / 32 * 32);
    }
    const uint32_t max_lf = std::min<uint32_t>(1u << max_log, (uint32_t)VB_THREADS);
    const size_t lds = std::max<size_t>((size_t)NL * 2 * max_lf, (size_t)NL * VB_THREADS) * 4;
    if (hi > lo) {
        VB_TRY(hipMemcpyAsync(set.c.as<uint8_t>() + lo, packed + lo, hi - lo, hipMemcpyHostToDevice, st_copy));
        VB_TRY(hipEventCreateWithFlags(&up, hipEventDisableTiming));
        VB_TRY(hipEventRecord(up, st_copy));
    }
    uint8_t* pz = small_pinned + b0 * 32;
    uint8_t* pm = small_pinned + nb * 32 + b0 * sizeof(VbBlob);
    memcpy(pz, zs + 4 * b0, (b1 - b0) * 32);
    memcpy(pm, meta + b0, (b1 - b0) * sizeof(VbBlob));
    VB_TRY(hipMemcpyAsync(d_zs + 2 * b0, pz, (b1 - b0) * 32, hipMemcpyHostToDevice, st));
    VB_TRY(hipMemcpyAsync(d_meta + b0, pm, (b1 - b0) * sizeof(VbBlob), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_vb_prep, dim3((unsigned)((b1 - b0 + 63) / 64)), dim3(64), 0, st, d_zs + 2 * b0, d_meta + b0, (uint32_t)(b1 - b0), d_prep + b0);
    if (up) {
        VB_TRY(hipStreamWaitEvent(st, up, 0));
        (void)hipEventDestroy(up);                                                     // released by the runtime once the wait has been satisfied
    }
    hipLaunchKernelGGL(k_vb_eval, dim3((unsigned)(b1 - b0)), dim3(VB_THREADS), lds, st, set.c.as<uint8_t>(), d_meta + b0, d_prep + b0, tb, d_ys + 2 * b0);
    VB_TRY(hipGetLastError());
#undef VB_TRY
    return KZG_OK;
}
int32_t vb_evaluate_finish(kzg_ctx* ctx, size_t nb, uint64_t* ys_out, uint8_t* fallback_out) {
    PolySet& set = ctx->poly[0];
    hipStream_t st = ctx->stream;
    uint4* d_ys = set.a.as<uint4>() + 2 * nb;
    VbPrep* d_prep = reinterpret_cast<VbPrep*>(set.b.as<VbBlob>() + nb);
    static thread_local std::vector<VbPrep> prep_host;
    prep_host.resize(nb);
    KZG_HIP_TRY(ctx, hipMemcpyAsync(ys_out, d_ys, nb * 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(prep_host.data(), d_prep, nb * sizeof(VbPrep), hipMemcpyDeviceToHost, st));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(st));
    for (size_t i = 0; i < nb; ++i) fallback_out[i] = prep_host[i].fallback ? 1 : 0;
    return KZG_OK;
}

}  // namespace kzg

#if defined(KZG_DEVICE_BOUND_CHECK)   // the device bound-check variant only (field29.h, `make boundcheck`)
#include "field29.h"
KZG_BOUND_CHECK_EXPORTS(vbeval)
#endif
