// provebatch.hip -- the batched prover: the proofs of many polynomials of one length in one launch sequence (capi_provebatch.hip drives it group
// by group; host_prove_batch.h plans the groups).  The reference proves one polynomial per call (KZG::compute_proof, prover/src/kzg.rs:128-178):
// n inversions, the quotient's n evaluations, one commitment over the Lagrange basis.  Here a group of `rows` polynomials of n = 2^log_n <= 2^12
// evaluations is
//   k_pb_rows_from_bytes   (bytes entries) big-endian blob bytes -> rows x n wire elements (helpers::to_fr_array, zero padding to n)
//   k_pb_prep              one LANE per row: z^n - 1 and the row's ONE inversion (none when z is on the domain)
//   k_pb_prove<M>          one WORKGROUP per row: y = f(z) and the quotient row q_j = (f_j - y) / (w^j - z) in one pass (provebatch_lanes.h)
//   commit_batch_device    the rows' quotients as ONE bucket problem over the cached Lagrange basis of n points
// z on the domain stays inside k_pb_prove (the identity in provebatch_lanes.h): no host search, no per-row call.
#include "poly_common.h"
#include "provebatch_lanes.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

namespace kzg {

static_assert(PB_MAX_LOG == PROVE_BATCH_MAX_LOG && PB_MAX_LOG == VB_MAX_LOG, "one largest class for the planner, the kernel and the descriptors");
static_assert(sizeof(PbPrep) <= 128, "PROVE_ROW_SMALL_BYTES counts 128 bytes for it");

// element i of row r = the 32 big-endian bytes [32 i, 32 i + 32) of blob r mod r, zero from the blob's last element on: k_blob_to_fr's arithmetic
// (poly.hip) on a packed group, every chunk whole (the packer zero-fills the last one), so every load is 128 bits wide
__global__ void __launch_bounds__(POLY_THREADS)
k_pb_rows_from_bytes(const uint8_t* __restrict__ packed, const VbBlob* __restrict__ meta, int log_n, uint32_t rows, uint4* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t r = idx >> log_n;
    if (r >= rows) return;
    const uint32_t i = (uint32_t)(idx & (((size_t)1 << log_n) - 1));
    const VbBlob b = meta[r];
    const uint32_t n_elems = (b.len + 31) / 32;
    uint32_t w32[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i < n_elems) be_chunk_load(w32, packed + b.off + (size_t)i * 32);
    Fr x, kk, v;
    fe_unpack(x, w32);
#pragma unroll
    for (int j = 0; j < NL; ++j) kk.l[j] = (int32_t)FrParams::K_RAW[j];       // 2^(256+261) mod r
    fe_mul(v, x, kk);                                                          // x * 2^256 mod r, in (-m, 2m)
    fe_canon(v);
    uint32_t o[8];
    fe_pack(o, v);
    out[2 * idx] = make_uint4(o[0], o[1], o[2], o[3]);
    out[2 * idx + 1] = make_uint4(o[4], o[5], o[6], o[7]);
}

__global__ void __launch_bounds__(64)
k_pb_prep(const uint32_t* __restrict__ zs_wire, int log_n, uint32_t rows, PbPrep* __restrict__ prep) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    Fr z;
    pb_wire_load(z, zs_wire, i);
    PbPrep o;
    pb_prep_lane(o, z, log_n);
    prep[i] = o;
}

// row = blockIdx.x; Lf = min(n, PB_THREADS) lanes carry M = n / Lf elements each; the launch has max(Lf, 64) lanes.
// Dynamic shared memory: NL planes of 2 Lf words, the product tree and then the block sums.
template <int M>
__global__ void __launch_bounds__(PB_THREADS)
k_pb_prove(const uint32_t* __restrict__ rows_wire, const PbPrep* __restrict__ prep, NttTables tb /* 2^PB_MAX_LOG domain */, int log_n,
           uint32_t* __restrict__ q_wire, uint32_t* __restrict__ ys_wire) {
    extern __shared__ int32_t tree[];
    __shared__ PbShared shared;
    const uint32_t n = 1u << log_n, Lf = n / (uint32_t)M, t = threadIdx.x;
    const int sh = PB_MAX_LOG - log_n;
    const size_t blob = blockIdx.x;
    const PbPrep& pr = prep[blob];
    const uint32_t* row = rows_wire + blob * n * 8;
    uint32_t* qrow = q_wire + blob * n * 8;
    const bool on_domain = pr.on_domain != 0;                    // uniform across the workgroup
    Fr z;
#pragma unroll
    for (int j = 0; j < NL; ++j) z.l[j] = pr.z[j];
    PbLane<M> lane;
    if (t < Lf) pb_lane_denominators(lane, tree, &shared, z, tb, t, Lf, sh);
    __syncthreads();
    for (uint32_t s = Lf >> 1; s >= 1; s >>= 1) {
        if (t < s) pb_tree_up(tree, Lf, s + t);
        __syncthreads();
    }
    if (t == 0) pb_tree_root(tree, Lf, pr);
    __syncthreads();
    for (uint32_t s = 1; s < Lf; s <<= 1) {
        if (t < s) pb_tree_down(tree, Lf, s + t);
        __syncthreads();
    }
    Fr sum;
    fe_set_zero(sum);
    if (t < Lf) pb_lane_terms(lane, sum, tree, &shared, row, tb, t, Lf, sh, on_domain);
    __syncthreads();                                             // the tree is dead: its planes carry the block sums
    if (!on_domain) {
        if (t < Lf) pb_sum_put(tree, Lf, t, sum);
        __syncthreads();
        int level = 0;
        for (uint32_t dd = Lf >> 1; dd >= 1; dd >>= 1, ++level) {
            if (t < dd) { pb_sum_step(tree, Lf, t, dd, level, sum); pb_sum_put(tree, Lf, t, sum); }
            __syncthreads();
        }
        if (t == 0) pb_finish_y(&shared, sum, pr, log_n);
        __syncthreads();
    }
    if (t == 0) pb_store_y(ys_wire, blob, &shared);
    if (t < Lf) pb_lane_quotient(lane, sum, &shared, qrow, tb, t, Lf, sh, on_domain);
    if (!on_domain) return;
    if (t < Lf) pb_sum_put(tree, Lf, t, sum);
    __syncthreads();
    int level = 0;
    for (uint32_t dd = Lf >> 1; dd >= 1; dd >>= 1, ++level) {
        if (t < dd) { pb_sum_step(tree, Lf, t, dd, level, sum); pb_sum_put(tree, Lf, t, sum); }
        __syncthreads();
    }
    if (t == 0) pb_store_q_m(qrow, sum, &shared, tb, n, sh);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
int32_t prove_batch_rows_from_bytes(kzg_ctx* ctx, const uint8_t* packed, size_t packed_bytes, const VbBlob* meta, size_t rows, int log_n, const void** d_rows) {
    const size_t n = (size_t)1 << log_n, bytes_al = (packed_bytes + 63) / 64 * 64;
    KZG_HIP_TRY(ctx, ctx->pb[0].reserve(bytes_al + rows * sizeof(VbBlob) + 64));
    KZG_HIP_TRY(ctx, ctx->pb[1].reserve(rows * n * 32 + 32));
    uint8_t* d_packed = ctx->pb[0].as<uint8_t>();
    VbBlob* d_meta = reinterpret_cast<VbBlob*>(d_packed + bytes_al);
    if (packed_bytes) KZG_HIP_TRY(ctx, hipMemcpyAsync(d_packed, packed, packed_bytes, hipMemcpyHostToDevice, ctx->stream));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(d_meta, meta, rows * sizeof(VbBlob), hipMemcpyHostToDevice, ctx->stream));
    const size_t total = rows * n;
    hipLaunchKernelGGL(k_pb_rows_from_bytes, dim3((unsigned)((total + POLY_THREADS - 1) / POLY_THREADS)), dim3(POLY_THREADS), 0, ctx->stream, d_packed, d_meta, log_n,
                       (uint32_t)rows, ctx->pb[1].as<uint4>());
    KZG_HIP_TRY(ctx, hipGetLastError());
    *d_rows = ctx->pb[1].p;
    return KZG_OK;
}

int32_t prove_batch_rows_run(kzg_ctx* ctx, kzg_srs* basis, const void* d_rows, int log_n, size_t rows, const uint64_t* zs, uint64_t* out_xy, uint8_t* out_inf,
                             uint64_t* out_ys) {
    if (rows == 0) return KZG_OK;
    if (log_n < 0 || log_n > PB_MAX_LOG || rows > PROVE_GROUP_ROWS_MAX) return KZG_ERR_INVALID_ARG;
    const size_t n = (size_t)1 << log_n;
    const uint32_t Lf = (uint32_t)std::min<size_t>(n, PB_THREADS);
    const int M = (int)(n / Lf);
    hipStream_t st = ctx->stream;
    NttTables tb;
    int32_t rc = ntt_get_tables(ctx, PB_MAX_LOG, false, &tb);
    if (rc != KZG_OK) return rc;
    KZG_HIP_TRY(ctx, ctx->pb[2].reserve(rows * n * 32 + 32));
    KZG_HIP_TRY(ctx, ctx->pb[3].reserve(rows * (32 + 32 + sizeof(PbPrep)) + 64));
    uint32_t* d_zs = ctx->pb[3].as<uint32_t>();
    uint32_t* d_ys = d_zs + rows * 8;
    PbPrep* d_prep = reinterpret_cast<PbPrep*>(d_ys + rows * 8);
    uint32_t* d_q = ctx->pb[2].as<uint32_t>();
    const bool trace = opts().vb_trace != 0;
    const auto t0 = Clock::now();
    KZG_HIP_TRY(ctx, hipMemcpyAsync(d_zs, zs, rows * 32, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pb_prep, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, st, d_zs, log_n, (uint32_t)rows, d_prep);
    const size_t lds = (size_t)NL * 2 * Lf * 4;
    const dim3 grid((unsigned)rows), block(std::max<uint32_t>(Lf, 64));
    const uint32_t* rw = static_cast<const uint32_t*>(d_rows);
    switch (M) {
        case 1: hipLaunchKernelGGL(k_pb_prove<1>, grid, block, lds, st, rw, d_prep, tb, log_n, d_q, d_ys); break;
        case 2: hipLaunchKernelGGL(k_pb_prove<2>, grid, block, lds, st, rw, d_prep, tb, log_n, d_q, d_ys); break;
        case 4: hipLaunchKernelGGL(k_pb_prove<4>, grid, block, lds, st, rw, d_prep, tb, log_n, d_q, d_ys); break;
        default: hipLaunchKernelGGL(k_pb_prove<8>, grid, block, lds, st, rw, d_prep, tb, log_n, d_q, d_ys); break;
    }
    KZG_HIP_TRY(ctx, hipGetLastError());
    static thread_local std::vector<uint64_t> ys_host;
    if (out_ys) {
        ys_host.resize(rows * 4);
        KZG_HIP_TRY(ctx, hipMemcpyAsync(ys_host.data(), d_ys, rows * 32, hipMemcpyDeviceToHost, st));
    }
    KZG_HIP_TRY(ctx, hipStreamSynchronize(st));                  // the commitments run on the slots' streams
    if (out_ys) memcpy(out_ys, ys_host.data(), rows * 32);
    const auto t1 = Clock::now();
    rc = commit_batch_device(ctx, basis, d_q, n, rows, out_xy, out_inf);
    if (trace)
        fprintf(stderr, "  prove_batch n=%zu rows=%zu: points up + prep + fused kernel %.3f ms, commitments of the quotient rows %.3f ms\n", n, rows, ms_between(t0, t1),
                ms_between(t1, Clock::now()));
    return rc;
}

}  // namespace kzg

#if defined(KZG_DEVICE_BOUND_CHECK)   // the device bound-check variant only (field29.h, `make boundcheck`)
#include "field29.h"
KZG_BOUND_CHECK_EXPORTS(provebatch)
#endif
