// host_encode.h — the host side of kzg_encode_cosets (multiproof.hip, capi_srs.hip): every argument check of the entry, in the order the
// header documents, and everything the driver decides before its first launch -- the sizes m, m', r, the shape of the FK20 linear
// combination, the workspace bytes, and the plan of the one transform that sees n: the m-point G1 FFT of an input that is zero beyond
// its first m' = m / r points.  Pure host code: no HIP type, no kzg_ctx, no allocation; also compiled with g++ by
// tests/hostcheck/encodecheck.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/kzg_bn254_mi355x.h"
#include "g1fft_plan.h"

namespace kzg {

constexpr size_t ENCODE_MAX_N = (size_t)1 << 24;
constexpr size_t ENCODE_FR_BYTES = 32;                          // one wire Fr
constexpr size_t ENCODE_AFFINE_BYTES = 64;                      // one wire affine point
constexpr size_t ENCODE_LIMBS = 9;                              // NL of field29.h: the affine conversion's scratch is NL words per point

// The shape of k_fk20_lincomb for chunk length l: G = 2^log_g <= 64 lanes of a wave per frequency, W <= 32 waves per frequency when
// l > 64, a lane adding tpl terms one after the other (l = G W tpl).  l = 1 runs k_fk20_pointwise instead.
struct Fk20Shape { int log_g; uint32_t W, tpl; };
inline Fk20Shape fk20_shape(size_t l) {
    Fk20Shape s;
    s.log_g = l >= 64 ? 6 : __builtin_ctzll(l);
    s.W = l > 64 ? (uint32_t)std::min<size_t>(l / 64, 32) : 1u;
    s.tpl = (uint32_t)(l / ((size_t)s.W << s.log_g));
    return s;
}

// The m-point forward transform of g1_fft_planes_padded: the input has `nonzero` = n / r points, the identity after them.
//   direct stages (n <= 2^14 by g1fft_choose_plan): the plan of g1_fft_planes with its copy replaced by a copy that pads;
//   radix-2: on bit-reversed input the non-zero points land on the multiples of r, and the first log2 r stages are butterflies
//   (A, 0) -> (A, A): one load planes[i] = in[bitrev(i >> log2 r)] stands for the bit reversal and those stages, and the stages
//   log2 r + 1 .. log2 n run unchanged.
// r = 1 is the plan of g1fft_plan_planes(n, false, false, true) itself.
struct G1fftPaddedPlan {
    G1fftPlan plan;
    uint32_t nonzero;
    int log_nonzero, log_r;
};
inline G1fftPaddedPlan g1fft_plan_planes_padded(size_t n, size_t nonzero) {
    G1fftPaddedPlan pp{};
    pp.plan = g1fft_plan_planes(n, false, false, true);
    pp.nonzero = (uint32_t)nonzero;
    pp.log_nonzero = g1fft_log2(nonzero);
    pp.log_r = pp.plan.log_n - pp.log_nonzero;
    if (pp.log_r == 0) return pp;
    G1fftPlan& p = pp.plan;
    if (p.form == G1FFT_RADIX2) {
        p.stage[0].kind = G1S_SPREAD_BITREV;
        p.stage[0].log_s = pp.log_r;                              // the stages the load stands for
        for (int i = 1; i + pp.log_r < p.n_stages; ++i) p.stage[i] = p.stage[i + pp.log_r];
        p.n_stages -= pp.log_r;
    } else {
        p.stage[0].kind = G1S_GATHER_PAD;
    }
    return pp;
}

// The checks of the header's table in their order.  Check 1 (null pointers, no output, proofs without flags) is `bad_pointers`; check 2
// (an SRS of another context, a Lagrange-basis handle) is `bad_srs`.
inline int32_t encode_check(bool bad_pointers, bool bad_srs, size_t poly_len, size_t n, size_t chunk_len, size_t srs_len) {
    if (bad_pointers) return KZG_ERR_INVALID_ARG;
    if (bad_srs) return KZG_ERR_INVALID_ARG;
    const size_t d = poly_len, l = chunk_len;
    if (d == 0 || (d & (d - 1)) != 0 || n == 0 || (n & (n - 1)) != 0) return KZG_ERR_NOT_POWER_OF_TWO;
    if (n > ENCODE_MAX_N) return KZG_ERR_DOMAIN;
    if (d > n || d == 1 || l == 0 || (l & (l - 1)) != 0 || l > d / 2) return KZG_ERR_INVALID_ARG;
    if (d > srs_len) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    return KZG_OK;
}

struct EncodePlan {
    size_t d = 0, n = 0, l = 0;
    size_t m = 0, mp = 0, r = 0, M = 0;    // cosets n / l, m' = d / l, the rate's inverse n / d = m / m', M' = 2 m'
    int log_d = 0, log_n = 0, log_l = 0, log_m = 0, log_r = 0;
    bool values = false, proofs = false;
    Fk20Shape lincomb{};
    // kzg_ctx::mp[0 .. 5]: coefficients, then evaluations | rows F^(b), then the coset-major values | three plane sets | affine points,
    // conversion scratch and flags
    size_t bytes[6] = {0, 0, 0, 0, 0, 0};
    G1fftPaddedPlan fft{};                 // step 5 (proofs only)
};

// The plan of a call whose arguments passed encode_check
inline EncodePlan encode_plan(size_t poly_len, size_t n, size_t chunk_len, bool values, bool proofs) {
    EncodePlan p;
    p.d = poly_len; p.n = n; p.l = chunk_len;
    p.m = n / chunk_len; p.mp = poly_len / chunk_len; p.r = n / poly_len; p.M = 2 * p.mp;
    p.log_d = g1fft_log2(p.d); p.log_n = g1fft_log2(n); p.log_l = g1fft_log2(p.l); p.log_m = p.log_n - p.log_l; p.log_r = p.log_n - p.log_d;
    p.values = values; p.proofs = proofs;
    p.lincomb = fk20_shape(p.l);
    p.bytes[0] = (values ? p.n : p.d) * ENCODE_FR_BYTES;                                  // the values are the NTT of the zero-extended coefficients, in place
    p.bytes[1] = std::max<size_t>(proofs ? 2 * p.d : 0, values ? p.n : 0) * ENCODE_FR_BYTES;      // FK20 rows sized by d; n x 32 B of values
    if (proofs) {
        const size_t set = std::max(p.M, p.m) * G1FFT_POINT_BYTES;                        // a plane set holds 2m' points of steps 3-4 and m of step 5
        p.bytes[2] = std::max(p.M * p.lincomb.W, p.m) * G1FFT_POINT_BYTES;
        p.bytes[3] = set;
        p.bytes[4] = set;
        p.bytes[5] = p.m * (ENCODE_AFFINE_BYTES + 1 + ENCODE_LIMBS * 4);
        p.fft = g1fft_plan_planes_padded(p.m, p.mp);
    }
    return p;
}

}  // namespace kzg
