// tests/devcheck/treecheck.hip -- TEST-ONLY stand-alone device check of group_sum_tree (csrc/curve_quad.h): the work-efficient tree behind the
// first level of the MSM bucket reduction, on its own, in both lane forms (pairs and quads), with one, two and four groups of 64 values per
// workgroup.  Arrays of 64 x {1, 3, 4, 5} points (with two or four groups per workgroup 1, 3, 5 leave a workgroup that is not full); slot 0 (the total) and the slots
// 2^k (the sum over the values whose index has bit k set) of every group are compared, as affine points, with host sums (host_curve.h).
// Inputs: random points; all identity; one non-identity value per group at slot 0, 1, 32, 63; for every step k the same point (P + P)
// and opposite points (P - P) at slots 0 and 2^k, so that the addition of step k doubles / cancels while other lanes of the wave add
// ordinary points; every slot equal (every addition of every step doubles).  Prints "treecheck ok" and returns 0, or the first mismatch.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "curve_quad.h"
#include "host_curve.h"

namespace {

using kzg::NL;
namespace H = kzg_host;

// wire XYZZ (32 words per point, identity = zeros) -> the 36 limb planes the reduction kernels read
__global__ void k_wire_to_planes(const uint32_t* __restrict__ wire, uint32_t n, int32_t* __restrict__ planes) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* w = wire + (size_t)i * 32;
    uint32_t any = 0;
    for (int j = 16; j < 24; ++j) any |= w[j];
    kzg::Xyzz v;
    if (any == 0) {
        kzg::xyzz_set_inf(v);
    } else {
        kzg::fe_from_wire(v.x, w);
        kzg::fe_from_wire(v.y, w + 8);
        kzg::fe_from_wire(v.zz, w + 16);
        kzg::fe_from_wire(v.zzz, w + 24);
        v.inf = false;
    }
    kzg::xyzz_store(planes, n, i, v);
}

// workgroup b: the groups [NG b, NG b + NG) of `planes` (n_groups x 64 values) -> out_wire[7 g + role], role k < 6 = slot 2^k, role 6 = slot 0
template <class LG, int NG>
__global__ void __launch_bounds__(64 * LG::LANES * NG) k_tree(const int32_t* __restrict__ planes, uint32_t n_groups, uint32_t* __restrict__ out_wire) {
    __shared__ int32_t lds[4 * NL * 64 * NG];
    const uint32_t lane = threadIdx.x & 63, t = threadIdx.x / LG::LANES;
    const typename LG::Role role = LG::role(lane);
    const uint32_t n = n_groups * 64, i = blockIdx.x * (64 * NG) + t;
    typename LG::Point v;
    LG::set_inf(v);
    if (i < n) LG::load(v, planes, n, i, role);          // (group-uniform)
    kzg::group_sum_tree<LG, NG>(v, t, role, lds);
    const uint32_t gr = t / 7, zr = t - gr * 7, g = blockIdx.x * NG + gr;
    if (gr >= (uint32_t)NG || g >= n_groups) return;
    LG::load(v, lds, 64 * NG, gr * 64 + (zr == 6 ? 0u : 1u << zr), role);
    LG::store_wire(out_wire, (size_t)g * 7 + zr, v, role);
}

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "treecheck: %s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
uint32_t rnd() { rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(rng_state >> 33); }

H::Xyzz generator() {
    H::Xyzz g;
    g.x = H::FQ_ONE;
    g.y = H::dbl(H::FQ_ONE);
    g.zz = H::FQ_ONE;
    g.zzz = H::FQ_ONE;
    return g;
}
// a pseudo-random multiple of the generator, left in whatever XYZZ form the double-and-add ends in (ZZ != 1)
H::Xyzz random_point() {
    const H::Xyzz g = generator();
    H::Xyzz acc = H::xyzz_inf();
    uint32_t s = rnd() | 0x40000001u;
    for (int b = 30; b >= 0; --b) {
        acc = H::xyzz_dbl(acc);
        if ((s >> b) & 1u) acc = H::xyzz_add(acc, g);
    }
    return acc;
}
H::Xyzz negate(const H::Xyzz& p) {
    H::Xyzz r = p;
    H::Fq zero;
    memset(&zero, 0, sizeof zero);
    r.y = H::sub(zero, p.y);
    return r;
}

struct Case { std::string name; std::vector<H::Xyzz> v; };

std::vector<Case> cases(uint32_t n_groups) {
    const uint32_t n = n_groups * 64;
    std::vector<Case> out;
    auto fresh = [&](const std::string& name, bool random) {
        Case c;
        c.name = name;
        c.v.assign(n, H::xyzz_inf());
        if (random) for (auto& p : c.v) p = random_point();
        out.push_back(c);
        return &out.back();
    };
    fresh("random points", true);
    fresh("all identity", false);
    for (uint32_t slot : {0u, 1u, 32u, 63u}) {
        Case* c = fresh("one value per group at slot " + std::to_string(slot), false);
        for (uint32_t g = 0; g < n_groups; ++g) c->v[g * 64 + slot] = random_point();
    }
    for (uint32_t k = 0; k < 6; ++k)
        for (int opposite = 0; opposite < 2; ++opposite) {
            // slot 0 enters step k as the sum of the slots below 2^k, slot 2^k as the sum of the slots [2^k, 2^(k+1)): P and +-P there, nothing else
            // below 2^(k+1), ordinary points above
            Case* c = fresh(std::string(opposite ? "opposite" : "equal") + " points at distance 2^" + std::to_string(k), true);
            for (uint32_t g = 0; g < n_groups; ++g) {
                for (uint32_t x = 0; x < (2u << k); ++x) c->v[g * 64 + x] = H::xyzz_inf();
                const H::Xyzz p = random_point();
                c->v[g * 64] = p;
                c->v[g * 64 + (1u << k)] = opposite ? negate(p) : p;
            }
        }
    {
        Case* c = fresh("every slot equal", false);
        for (uint32_t g = 0; g < n_groups; ++g) {
            const H::Xyzz p = random_point();
            for (uint32_t x = 0; x < 64; ++x) c->v[g * 64 + x] = p;
        }
    }
    return out;
}

template <class LG, int NG>
int run_form(const char* form) {
    int bad = 0;
    for (uint32_t n_groups : {1u, 3u, 4u, 5u}) {
        const uint32_t n = n_groups * 64, n_res = n_groups * 7;
        uint32_t* d_wire;
        uint32_t* d_out;
        int32_t* d_planes;
        HIP_OK(hipMalloc(&d_wire, (size_t)n * 128));
        HIP_OK(hipMalloc(&d_planes, (size_t)n * 36 * 4));
        HIP_OK(hipMalloc(&d_out, (size_t)n_res * 128));
        for (const Case& c : cases(n_groups)) {
            static_assert(sizeof(H::Xyzz) == 128, "XYZZ wire words");
            HIP_OK(hipMemcpy(d_wire, c.v.data(), (size_t)n * 128, hipMemcpyHostToDevice));
            HIP_OK(hipMemset(d_out, 0xFF, (size_t)n_res * 128));
            hipLaunchKernelGGL(k_wire_to_planes, dim3((n + 63) / 64), dim3(64), 0, 0, d_wire, n, d_planes);
            hipLaunchKernelGGL((k_tree<LG, NG>), dim3((n_groups + NG - 1) / NG), dim3(64 * LG::LANES * NG), 0, 0, d_planes, n_groups, d_out);
            HIP_OK(hipGetLastError());
            std::vector<H::Xyzz> got(n_res);
            HIP_OK(hipMemcpy(got.data(), d_out, (size_t)n_res * 128, hipMemcpyDeviceToHost));
            for (uint32_t g = 0; g < n_groups; ++g)
                for (uint32_t role = 0; role < 7; ++role) {
                    H::Xyzz want = H::xyzz_inf();
                    for (uint32_t x = 0; x < 64; ++x)
                        if (role == 6 || ((x >> role) & 1u)) want = H::xyzz_add(want, c.v[g * 64 + x]);
                    uint64_t a[8], b[8];
                    uint8_t ia = 0, ib = 0;
                    H::xyzz_to_affine(got[g * 7 + role], a, &ia);
                    H::xyzz_to_affine(want, b, &ib);
                    if (ia != ib || memcmp(a, b, 64) != 0) {
                        if (bad++ < 8) fprintf(stderr, "treecheck: %s, %d groups per workgroup, %u groups, %s: group %u role %u differs (identity %d, want %d)\n", form, NG, n_groups, c.name.c_str(), g, role, ia, ib);
                    }
                }
        }
        HIP_OK(hipFree(d_wire));
        HIP_OK(hipFree(d_planes));
        HIP_OK(hipFree(d_out));
    }
    return bad;
}

}  // namespace

int main() {
    const int bad = run_form<kzg::PairLanes, 1>("pairs") + run_form<kzg::PairLanes, 2>("pairs") + run_form<kzg::PairLanes, 4>("pairs") +
                    run_form<kzg::QuadLanes, 1>("quads") + run_form<kzg::QuadLanes, 2>("quads") + run_form<kzg::QuadLanes, 4>("quads");
    if (bad) { fprintf(stderr, "treecheck: %d sums differ\n", bad); return 1; }
    printf("treecheck ok\n");
    return 0;
}
