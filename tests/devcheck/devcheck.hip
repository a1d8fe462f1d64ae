// tests/devcheck/devcheck.hip -- TEST-ONLY device conformance kernels for the field layer (csrc/field29.h, fe_asm.h, fe_invert.h),
// loaded by tests/test_gpu_device_math.py.  Not part of the product library.
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

typedef void (*Kernel)(const int32_t*, int32_t*, uint32_t);

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

}  // extern "C"

KZG_BOUND_CHECK_EXPORTS(devcheck)
