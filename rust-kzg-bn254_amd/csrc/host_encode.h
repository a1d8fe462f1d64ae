// host_encode.h — the host side of kzg_encode_cosets (multiproof.hip, capi_srs.hip): every argument check of the entry, in the order the
// header documents, and everything the driver decides before its first launch -- the sizes m, m', r, the shape of the FK20 linear
// combination, the workspace bytes, and the plan of the one transform that sees n: the m-point G1 FFT of an input that is zero beyond
// its first m' = m / r points -- and of kzg_encode_cosets_batch: its checks, the groups a call works through, the bytes of a group, and
// both G1 transform plans chosen for the blobs of a group (EncodeBatchPlan, below).  Pure host code: no HIP type, no kzg_ctx, no allocation; also compiled with g++ by
// tests/hostcheck/encodecheck.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/kzg_bn254_mi355x.h"
#include "g1fft_plan.h"
#include "ntt_plan.h"

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
// batch: transforms per launch, as in g1fft_plan_planes.
inline G1fftPaddedPlan g1fft_plan_planes_padded(size_t n, size_t nonzero, size_t batch = 1) {
    G1fftPaddedPlan pp{};
    pp.plan = g1fft_plan_planes(n, false, false, true, batch);
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

// ---- kzg_encode_cosets_batch: `count` blobs of one shape (d, n, l, form) --------------------------------------------------------------
// A call works through its blobs in GROUPS.  Inside a group every stage of the encoder is one launch for all its blobs: the blob is
// grid.y of the kernel, and the blobs' buffers stand one after the other in each kzg_ctx::mp[i], a fixed distance apart (blob_bytes[i]
// apart for the plane sets; the Fr arrays are compact rows, see below).  A group of one blob runs the launches of kzg_encode_cosets
// itself (multiproof_encode), so the batched entry is never slower than the loop where batching cannot help.
//
// The default budget of a group's workspace: 4 GiB.  From the shapes of profiles/encode.md: one blob needs ~3 MiB at (2^12, r = 8,
// l = 16), ~50 MiB at (2^16, 8, 16), the largest l = 16 row, and ~300 MiB at (2^16, 8, 1), the largest row: 4 GiB holds 64 blobs of
// every l = 16 row in one group and 13 of the largest, 1.4 % of the device's 288 GB.  kzg_ctx_set_encode_group_bytes overrides it.
constexpr size_t ENCODE_GROUP_BYTES_DEFAULT = (size_t)4 << 30;
constexpr size_t ENCODE_GROUP_MAX = 32768;                      // blobs per group: grid.y of a launch (< 65 536)
constexpr size_t ENCODE_STAGE_LANE_CAP = 65536;                 // one wave per SIMD: g1fft_choose_plan's cap

// kzg_encode_cosets_batch's checks: encode_check with count == 0 in check 1 and, last, a count whose output sizes overflow size_t
inline int32_t encode_batch_check(bool bad_pointers, bool bad_srs, size_t count, size_t poly_len, size_t n, size_t chunk_len, size_t srs_len) {
    int32_t rc = encode_check(bad_pointers || count == 0, bad_srs, poly_len, n, chunk_len, srs_len);
    if (rc != KZG_OK) return rc;
    // the largest array is max(n x 32 (values), m x 64 (proofs)) <= n x 64 bytes per blob
    if (count > SIZE_MAX / (n * ENCODE_AFFINE_BYTES)) return KZG_ERR_INVALID_ARG;
    return KZG_OK;
}

// the smallest number of lanes of a stage of the plan that multiplies points (direct and radix-2 stages), one transform
inline size_t g1fft_plan_min_stage_lanes(const G1fftPlan& p) {
    size_t lanes = SIZE_MAX;
    for (int i = 0; i < p.n_stages; ++i)
        if (p.stage[i].K > 0) lanes = std::min(lanes, p.stage[i].grid * 256);
    return lanes;
}

struct EncodeBatchPlan {
    EncodePlan one;                        // the plan of one blob: the shape, and the launches of a group of one
    size_t count = 0;
    // THE RULE for when batching cannot help: a stage is pure latency only while it fits one wave per SIMD (ENCODE_STAGE_LANE_CAP lanes);
    // beyond that it is throughput bound and B blobs in one launch take B times as long as one.  When proofs are asked for and EVERY
    // scalar-multiplication stage of ONE blob (the linear combination, each stage of the inverse and of the forward G1 FFT) already has
    // that many lanes, `batched` is false and the call runs as groups of one.  Values alone (Fr NTTs only) always batch.
    bool batched = false;
    size_t min_stage_lanes = 0;            // the smallest of those stages of one blob (0: no proofs)
    size_t group = 1;                      // blobs per group (the last group of a call may be smaller): >= 1 whatever the budget
    size_t n_groups = 0;
    size_t budget = 0;                     // the byte budget the group was sized for
    size_t f_stride = 0;                   // Fr elements between the coefficient rows of consecutive blobs in mp[0]: n with values, else d
    // bytes of kzg_ctx::mp[0 .. 5] per blob and per group, and of the Fr NTT workspace (mp_ntt.data, .tmp) per group
    size_t blob_bytes[6] = {0, 0, 0, 0, 0, 0}, bytes[6] = {0, 0, 0, 0, 0, 0};
    size_t ntt_bytes[2] = {0, 0};
    size_t group_bytes = 0;                // everything a group reserves
    size_t set_points[3] = {0, 0, 0};      // points per blob of the three plane sets mp[2 .. 4]
    G1fftPlan ifft{};                      // steps 3: the inverse transform of 2m' points, chosen for `group` blobs per launch
    G1fftPaddedPlan fft{};                 // step 5: the zero-padded forward transform of m points, likewise
};

// Fr NTT workspace of `rows` transforms of 2^log_n points in one launch per pass (ntt_run_batch): ntt_plan's bytes times the rows
inline void encode_ntt_bytes(int log_n, size_t rows, size_t out[2]) {
    if (log_n < 1) return;
    const NttPlan p = ntt_plan(log_n, false, 256, 0);           // the byte counts depend on log n only
    out[0] = std::max(out[0], p.bytes_data * rows);
    out[1] = std::max(out[1], p.bytes_tmp * rows);
}

// The sizes and the two transform plans of a group of g blobs (1 <= g)
inline void encode_batch_size_group(EncodeBatchPlan& bp, size_t g) {
    const EncodePlan& p = bp.one;
    bp.group = g;
    bp.group_bytes = 0;
    for (int i = 0; i < 6; ++i) { bp.bytes[i] = bp.blob_bytes[i] * g; bp.group_bytes += bp.bytes[i]; }
    bp.ntt_bytes[0] = bp.ntt_bytes[1] = 0;
    if (p.proofs) encode_ntt_bytes(g1fft_log2(p.M), p.l * g, bp.ntt_bytes);      // the l g rows of 2m' points
    if (p.values) encode_ntt_bytes(p.log_n, g, bp.ntt_bytes);                    // the g value transforms
    encode_ntt_bytes(p.log_d, g, bp.ntt_bytes);                                  // eval form: the g inverse transforms of d points
    bp.group_bytes += bp.ntt_bytes[0] + bp.ntt_bytes[1];
    if (p.proofs) {
        bp.ifft = g1fft_plan_planes(p.M, true, true, false, g);
        bp.fft = g1fft_plan_planes_padded(p.m, p.mp, g);
    }
}

// The plan of a call whose arguments passed encode_batch_check.  group_bytes = 0: the default budget.
inline EncodeBatchPlan encode_batch_plan(size_t poly_len, size_t n, size_t chunk_len, size_t count, bool values, bool proofs, size_t group_bytes) {
    EncodeBatchPlan bp;
    bp.one = encode_plan(poly_len, n, chunk_len, values, proofs);
    const EncodePlan& p = bp.one;
    bp.count = count;
    bp.budget = group_bytes ? group_bytes : ENCODE_GROUP_BYTES_DEFAULT;
    bp.f_stride = values ? p.n : p.d;
    for (int i = 0; i < 6; ++i) bp.blob_bytes[i] = p.bytes[i];
    if (proofs) {
        for (int i = 0; i < 3; ++i) bp.set_points[i] = p.bytes[2 + i] / G1FFT_POINT_BYTES;
        const size_t lincomb = p.l == 1 ? p.M : ((p.M * p.lincomb.W) << p.lincomb.log_g);
        bp.min_stage_lanes = std::min(lincomb, std::min(g1fft_plan_min_stage_lanes(g1fft_plan_planes(p.M, true, true, false)),
                                                        g1fft_plan_min_stage_lanes(g1fft_plan_planes_padded(p.m, p.mp).plan)));
    }
    bp.batched = !proofs || bp.min_stage_lanes < ENCODE_STAGE_LANE_CAP;
    size_t g = 1;
    if (bp.batched && count > 1) {
        encode_batch_size_group(bp, 1);
        // the workspace is linear in the blobs of the group (the transform plans own no bytes): the largest g within the budget
        const size_t per_blob = std::max<size_t>(bp.group_bytes, 1);
        g = std::min(std::min(count, ENCODE_GROUP_MAX), std::max<size_t>(1, bp.budget / per_blob));
    }
    encode_batch_size_group(bp, g);
    bp.n_groups = (count + g - 1) / g;
    return bp;
}

}  // namespace kzg
