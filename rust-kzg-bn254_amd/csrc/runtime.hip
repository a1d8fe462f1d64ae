// runtime.hip — what every unit of the library shares at run time and no kernel: the environment (opts()), the roctx ranges, the error
// text of a context, the host pool behind host_parallel_for, and (bound-check variant only) the totals over every unit's counters.
#include "engine.h"
#include "host_pool.h"

#include <cstdio>
#include <cstdlib>
#include <dlfcn.h>

namespace kzg {

// roctx ranges through dlopen (engine.h)
namespace {
struct RoctxApi {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    RoctxApi() {
        if (!opts().roctx) return;
        void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return;
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (!push || !pop) { push = nullptr; pop = nullptr; }
    }
};
const RoctxApi& roctx_api() { static const RoctxApi api; return api; }
}  // namespace
void roctx_push(const char* name) { const RoctxApi& a = roctx_api(); if (a.push) (void)a.push(name); }
void roctx_pop() { const RoctxApi& a = roctx_api(); if (a.pop) (void)a.pop(); }

// ---- the environment variables of the library, all of them (engine.h Opts; documented in the header and in INTEGRATION.md) ------------------
static int env_int(const char* name, int dflt) { const char* e = getenv(name); return e && *e ? atoi(e) : dflt; }
const Opts& opts() {
    static const Opts o = []() {
        Opts v;
        v.host_threads_max = env_int("KZG_HOST_THREADS_MAX", 0);
        v.host_threads = env_int("KZG_HOST_THREADS", 0);
        v.vb_trace = env_int("KZG_VB_TRACE", 0);
        { const char* e = getenv("KZG_VB_GROUP_BYTES"); v.vb_group_bytes = e && atol(e) > 0 ? (size_t)atol(e) : 0; }
        { const char* e = getenv("KZG_VB_CHUNK_BYTES"); v.vb_chunk_bytes = e && atol(e) > 0 ? (size_t)atol(e) : 0; }
        v.roctx = env_int("KZG_ROCTX", 0) != 0;
        { const char* e = getenv("KZG_EXCHANGE_TIMEOUT_S"); const double t = e ? atof(e) : 60.0; v.exchange_timeout_s = t > 0 ? t : 60.0; }
        { const char* e = getenv("KZG_RCCL_LIB"); v.rccl_lib = e && *e ? e : nullptr; }
        v.ntt_tile_log = env_int("KZG_NTT_TILE_LOG", 0);
        return v;
    }();
    return o;
}
bool opt_no_precompute() { return env_int("KZG_NO_PRECOMPUTE", 0) != 0; }
bool opt_no_naf() { return env_int("KZG_NO_NAF", 0) != 0; }

int32_t set_error(kzg_ctx* ctx, hipError_t e, const char* where) {
    if (ctx) {
        char buf[512];
        snprintf(buf, sizeof buf, "%s: %s", where, hipGetErrorString(e));
        ctx->last_error = buf;
    }
    (void)hipGetLastError();
    return KZG_ERR_DEVICE;
}

// The pool's two overrides are read here, once: host_pool.h itself knows nothing of the environment.
unsigned host_pool_threads(size_t jobs) {
    static const unsigned cap = kzg_host::host_threads_cap(opts().host_threads_max);
    return kzg_host::host_threads(jobs, cap, opts().host_threads);
}
void host_parallel_for(size_t n, const std::function<void(size_t)>& job) { kzg_host::HostPool::get().run(host_pool_threads(n), n, job); }

}  // namespace kzg

#if defined(KZG_DEVICE_BOUND_CHECK)
#include "field29.h"
KZG_BOUND_CHECK_EXPORTS(runtime)
// The variant library's totals over every translation unit: counts[site] summed, first[site] = the operand limbs kept by the first
// translation unit (in the order below) whose counter of that site fired.  Not declared in include/kzg_bn254_mi355x.h.
#define KZG_BC_UNITS(X) X(msm) X(ntt) X(poly) X(vbeval) X(lagrange) X(srs) X(g1fft) X(capi) X(capi_srs) X(capi_verify) X(capi_coset) X(runtime) X(blobstream) X(multi) X(ubench) X(multiproof) X(multiverify) X(multilocate) X(recover) X(g2msm) X(g2batch) X(g2decode) X(capi_g2) X(fsdevice) X(cosetbytes) X(capi_bytes) X(provecosets) X(capi_prove) X(pairing) X(provebatch) X(capi_provebatch)
#define KZG_BC_DECLARE(name) extern "C" int kzg_bc_read_##name(unsigned long long*, int32_t*); extern "C" int kzg_bc_reset_##name();
KZG_BC_UNITS(KZG_BC_DECLARE)
extern "C" int kzg_bc_sites() { return kzg::KZG_SITES; }
extern "C" int kzg_bc_read_all(unsigned long long* counts, int32_t* first) {
    unsigned long long c[kzg::KZG_SITES];
    int32_t f[kzg::KZG_SITES][kzg::NL];
    for (int s = 0; s < kzg::KZG_SITES; ++s) counts[s] = 0;
    int rc = 0;
#define KZG_BC_READ(name)                                                                                            \
    if (kzg_bc_read_##name(c, &f[0][0]) != 0) rc = -1;                                                               \
    for (int s = 0; s < kzg::KZG_SITES; ++s) {                                                                       \
        if (c[s] && !counts[s])                                                                                      \
            for (int j = 0; j < kzg::NL; ++j) first[s * kzg::NL + j] = f[s][j];                                      \
        counts[s] += c[s];                                                                                           \
    }
    KZG_BC_UNITS(KZG_BC_READ)
    return rc;
}
extern "C" int kzg_bc_reset_all() {
    int rc = 0;
#define KZG_BC_RESET(name) if (kzg_bc_reset_##name() != 0) rc = -1;
    KZG_BC_UNITS(KZG_BC_RESET)
    return rc;
}
#endif
