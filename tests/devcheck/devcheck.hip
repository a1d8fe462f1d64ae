// tests/devcheck/devcheck.hip -- TEST-ONLY device conformance kernels for the field layer (csrc/field29.h, fe_asm.h, fe_invert.h),
// the point formulas and the GLV scalar multiplications (dc_glv.h), loaded by tests/test_gpu_device_math.py and tests/test_gpu_glv.py.
// Not part of the product library.
//
// Each kernel applies ONE primitive of dc_prims.h elementwise, one element per lane, so the generated inline-asm products run at every
// lane and wave position of a full-chip launch.  The file is compiled several times into one library, each time with its own prefix
// for the exported names (DC_PREFIX) and its own namespace for the kernels (DC_NS):
//   dc_asm_  as the product builds it (the inline-asm products of fe_asm.h),
//   dc_cpp_  with -DKZG_NO_FE_ASM (the C++ forms of field29.h on the device),
//   dc_bc_   with -DKZG_DEVICE_BOUND_CHECK (the device bound-check counters; positive control of the checker).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dc_prims.h"
#include "dc_glv.h"

#ifndef DC_PREFIX
#define DC_PREFIX dc_asm_
#define DC_NS dc_asm
#endif
#define DC_CAT2(a, b) a##b
#define DC_CAT(a, b) DC_CAT2(a, b)
#define DC(name) DC_CAT(DC_PREFIX, name)

namespace DC_NS {
using namespace kzg;

template <class F, int OP>
__global__ __launch_bounds__(256) void k_prim(const int32_t* __restrict__ in, int32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t x[4 * NL], y[2 * NL];
#pragma unroll
    for (int j = 0; j < 4 * NL; ++j) x[j] = in[(size_t)i * (4 * NL) + j];
    dc_apply<F>(OP, x, y);
#pragma unroll
    for (int j = 0; j < 2 * NL; ++j) out[(size_t)i * (2 * NL) + j] = y[j];
}

template <int OP>
__global__ __launch_bounds__(256) void k_curve(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t x[33], y[32];
    for (int j = 0; j < 33; ++j) x[j] = in[(size_t)i * 33 + j];
    dc_curve(OP, x, y);
    for (int j = 0; j < 32; ++j) out[(size_t)i * 32 + j] = y[j];
}

__global__ __launch_bounds__(256) void k_naf(const uint32_t* __restrict__ in, const int32_t* __restrict__ width, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t x[8], y[64] = {};
    for (int j = 0; j < 8; ++j) x[j] = in[(size_t)i * 8 + j];
    dc_naf(x, width[i], y);
    for (int j = 0; j < 64; ++j) out[(size_t)i * 64 + j] = y[j];
}

__global__ __launch_bounds__(256) void k_glv(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    dc_glv(in + (size_t)i * 8, out + (size_t)i * 8);
}

// The lane-form kernels: the launch covers whole workgroups of valid rows (dc_launch_padded), so no lane leaves before the chain.
template <int FORM>
__global__ __launch_bounds__(256) void k_smul(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, row = t / dc_form_lanes(FORM), role = t % dc_form_lanes(FORM);
    uint32_t x[DC_SMUL_IN];
    for (int j = 0; j < DC_SMUL_IN; ++j) x[j] = in[(size_t)row * DC_SMUL_IN + j];
    dc_smul<FORM>(x, out, row, role);
}

template <int FORM, int OP>
__global__ __launch_bounds__(256) void k_lanes_curve(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, row = t / dc_form_lanes(FORM), role = t % dc_form_lanes(FORM);
    uint32_t x[DC_CURVE_IN];
    for (int j = 0; j < DC_CURVE_IN; ++j) x[j] = in[(size_t)row * DC_CURVE_IN + j];
    dc_lanes_curve<FORM, OP>(x, out, row, role);
}

typedef void (*Kernel)(const int32_t*, int32_t*, uint32_t);
typedef void (*RowKernel)(const uint32_t*, uint32_t*);

template <class F, int OP>
static Kernel pick_op(int op) {
    if constexpr (OP < DC_OPS) return op == OP ? k_prim<F, OP> : pick_op<F, OP + 1>(op);
    else return nullptr;
}
}  // namespace DC_NS

extern "C" {

int DC(ops)() { return kzg::DC_OPS; }

// which: 0 = Fq, 1 = Fr.  in: n x 36 int32, out: n x 18 int32 (host memory).  One launch of ceil(n / 256) workgroups of 256 lanes.
// Returns 0, or a HIP error code (-1: unknown op).
int DC(run)(int which, int op, const int32_t* in, int32_t* out, uint32_t n) {
    DC_NS::Kernel k = which == 0 ? DC_NS::pick_op<kzg::FqParams, 0>(op) : DC_NS::pick_op<kzg::FrParams, 0>(op);
    if (!k) return -1;
    if (n == 0) return 0;
    int32_t *din = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc(&din, (size_t)n * 36 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&dout, (size_t)n * 18 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(din, in, (size_t)n * 36 * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0xA5, (size_t)n * 18 * sizeof(int32_t));   // a lane that writes nothing cannot pass
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k, dim3((n + 255) / 256), dim3(256), 0, 0, din, dout, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * 18 * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return (int)e;
}

// curve op (DcCurveOp): in n x 33 u32, out n x 32 u32.  naf: in n x 8 u32 scalars, width n x int32, out n x 64 u32.
static int dc_launch(const void* in, size_t in_bytes, const void* in2, size_t in2_bytes, void* out, size_t out_bytes, uint32_t n, int what) {
    void *din = nullptr, *din2 = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc(&din, in_bytes);
    if (e == hipSuccess && in2) e = hipMalloc(&din2, in2_bytes);
    if (e == hipSuccess) e = hipMalloc(&dout, out_bytes);
    if (e == hipSuccess) e = hipMemcpy(din, in, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && in2) e = hipMemcpy(din2, in2, in2_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0xA5, out_bytes);
    if (e == hipSuccess) {
        const dim3 g((n + 255) / 256), b(256);
        const uint32_t* i32 = (const uint32_t*)din;
        uint32_t* o32 = (uint32_t*)dout;
        if (what == kzg::DC_MADD) hipLaunchKernelGGL(DC_NS::k_curve<kzg::DC_MADD>, g, b, 0, 0, i32, o32, n);
        else if (what == kzg::DC_PADD) hipLaunchKernelGGL(DC_NS::k_curve<kzg::DC_PADD>, g, b, 0, 0, i32, o32, n);
        else if (what == kzg::DC_PDBL) hipLaunchKernelGGL(DC_NS::k_curve<kzg::DC_PDBL>, g, b, 0, 0, i32, o32, n);
        else hipLaunchKernelGGL(DC_NS::k_naf, g, b, 0, 0, i32, (const int32_t*)din2, o32, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (din2) (void)hipFree(din2);
    if (dout) (void)hipFree(dout);
    return (int)e;
}
int DC(curve)(int op, const uint32_t* in, uint32_t* out, uint32_t n) {
    if (op < 0 || op >= kzg::DC_CURVE_OPS) return -1;
    return n ? dc_launch(in, (size_t)n * 33 * 4, nullptr, 0, out, (size_t)n * 32 * 4, n, op) : 0;
}
int DC(naf)(const uint32_t* scalars, const int32_t* width, uint32_t* out, uint32_t n) {
    return n ? dc_launch(scalars, (size_t)n * 32, width, (size_t)n * 4, out, (size_t)n * 64 * 4, n, -1) : 0;
}

// kk = glv_decompose(k): k n x 8 u32 (canonical scalars), kk n x 8 u32.  One lane per row.
int DC(glv)(const uint32_t* k, uint32_t* kk, uint32_t n) {
    if (n == 0) return 0;
    uint32_t *din = nullptr, *dout = nullptr;
    const size_t bytes = (size_t)n * 8 * sizeof(uint32_t);
    hipError_t e = hipMalloc(&din, bytes);
    if (e == hipSuccess) e = hipMalloc(&dout, bytes);
    if (e == hipSuccess) e = hipMemcpy(din, k, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0xA5, bytes);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(DC_NS::k_glv, dim3((n + 255) / 256), dim3(256), 0, 0, din, dout, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(kk, dout, bytes, hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return (int)e;
}

// One row per `lanes` adjacent lanes, in whole workgroups: the rows are padded to a multiple of 256 / lanes with copies of the first rows
// (valid rows: every lane of every wave runs the chain), both buffers hold the padded count, and only the n real rows come back.
static int dc_launch_padded(DC_NS::RowKernel kernel, uint32_t lanes, const uint32_t* in, size_t in_words, uint32_t* out, size_t out_words, uint32_t n) {
    const size_t per_wg = 256 / lanes, np = ((size_t)n + per_wg - 1) / per_wg * per_wg;
    uint32_t *din = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc(&din, np * in_words * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&dout, np * out_words * sizeof(uint32_t));
    for (size_t done = 0; e == hipSuccess && done < np;) {
        const size_t chunk = np - done < n ? np - done : n;
        e = hipMemcpy(din + done * in_words, in, chunk * in_words * sizeof(uint32_t), hipMemcpyHostToDevice);
        done += chunk;
    }
    if (e == hipSuccess) e = hipMemset(dout, 0xA5, np * out_words * sizeof(uint32_t));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)(np / per_wg)), dim3(256), 0, 0, (const uint32_t*)din, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * out_words * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return (int)e;
}

// form (DcForm): 0 one lane, 1 lane pair, 2 lane quad per row.  in: n x 40 u32 (P1, P2 affine wire points, then the halves kk), out: n x 32 u32
// XYZZ wire words of [kk] (P1 + P2).  Returns 0, or a HIP error code (-1: unknown form).
int DC(smul)(int form, const uint32_t* in, uint32_t* out, uint32_t n) {
    using namespace kzg;
    if (form < 0 || form >= DC_FORMS) return -1;
    if (n == 0) return 0;
    const DC_NS::RowKernel k = form == DC_LANE ? DC_NS::k_smul<DC_LANE> : form == DC_PAIR ? DC_NS::k_smul<DC_PAIR> : DC_NS::k_smul<DC_QUAD>;
    return dc_launch_padded(k, dc_form_lanes(form), in, DC_SMUL_IN, out, DC_POINT_OUT, n);
}

// form 1 or 2, op (DcCurveOp): the rows and semantics of DC(curve) through the lane-form formulas.  in: n x 33 u32, out: n x 32 u32.
int DC(lanes_curve)(int form, int op, const uint32_t* in, uint32_t* out, uint32_t n) {
    using namespace kzg;
    if ((form != DC_PAIR && form != DC_QUAD) || op < 0 || op >= DC_CURVE_OPS) return -1;
    if (n == 0) return 0;
    static const DC_NS::RowKernel ks[2][3] = {
        {DC_NS::k_lanes_curve<DC_PAIR, DC_MADD>, DC_NS::k_lanes_curve<DC_PAIR, DC_PADD>, DC_NS::k_lanes_curve<DC_PAIR, DC_PDBL>},
        {DC_NS::k_lanes_curve<DC_QUAD, DC_MADD>, DC_NS::k_lanes_curve<DC_QUAD, DC_PADD>, DC_NS::k_lanes_curve<DC_QUAD, DC_PDBL>}};
    return dc_launch_padded(ks[form - DC_PAIR][op], dc_form_lanes(form), in, DC_CURVE_IN, out, DC_POINT_OUT, n);
}

}  // extern "C"

KZG_BOUND_CHECK_EXPORTS(devcheck)
