// tests/devcheck/dc_glv.h -- TEST-ONLY, device only (included by devcheck.hip alone: glv.h is __device__ code, dc_prims.h is shared with the
// g++ host build): the GLV decomposition and the three GLV scalar multiplications (csrc/glv.h, csrc/glv_lanes.h), and the point formulas
// of the lane-pair and lane-quad forms (csrc/curve_pair.h, csrc/curve_quad.h), one row per lane, lane pair or lane quad.
//
// The lane forms use __all and DPP moves, and the product never calls them from a partly exited wave: every function here runs in EVERY
// lane of the launch (the exports of devcheck.hip pad the rows to whole workgroups with valid rows), and nothing returns early.
#pragma once
#include "dc_prims.h"
#include "glv.h"
#include "glv_lanes.h"

namespace kzg {

enum DcForm { DC_LANE, DC_PAIR, DC_QUAD, DC_FORMS };
constexpr int DC_SMUL_IN = 40, DC_POINT_OUT = 32, DC_CURVE_IN = 33;

constexpr uint32_t dc_form_lanes(int form) { return form == DC_LANE ? 1u : form == DC_PAIR ? 2u : 4u; }

// the point as half_load delivers it from memory: the even lane (X, ZZ), the odd lane (Y, ZZZ); the identity is literal zeros
__device__ __forceinline__ void dc_half_pick(HalfXyzz& h, const Xyzz& p, bool odd) {
    fe_select(h.u, odd, p.y, p.x);
    fe_select(h.v, odd, p.zzz, p.zz);
    h.inf = p.inf;
    if (p.inf) half_set_inf(h);
}
// ... and as quad_load delivers it: coordinate q in lane q
__device__ __forceinline__ void dc_quad_pick(QuadXyzz& h, const Xyzz& p, uint32_t q) {
    quad_pick(h, p, q);
    if (p.inf) quad_set_inf(h);
}

// kk = glv_decompose(k): 8 words in, 8 words out
__device__ __forceinline__ void dc_glv(const uint32_t* in, uint32_t* out) {
    uint32_t k[8], kk[8];
    for (int j = 0; j < 8; ++j) k[j] = in[j];
    glv_decompose(kk, k);
    for (int j = 0; j < 8; ++j) out[j] = kk[j];
}

// The base point of a scalar-multiplication row, P1 + P2 by xyzz_madd exactly as dc_curve builds its operand: stored-form coordinates in
// their lazy ranges with ZZ != 1 (P1 = identity: the affine P2 itself; P1 = -P2: the identity).  P2 is never the identity.
__device__ __forceinline__ void dc_smul_base(Xyzz& a, const uint32_t* in) {
    Affine p1, p2;
    const bool has1 = dc_load_point(p1, in);
    dc_load_point(p2, in + 16);
    if (has1) xyzz_from_affine(a, p1, 0); else xyzz_set_inf(a);
    xyzz_madd(a, p2, 0);
    if (a.inf) xyzz_set_inf(a);
}

// out row `row` = [kk] (P1 + P2), kk = in[32 .. 40) given as halves; `role` = lane within the pair / quad
template <int FORM>
__device__ __forceinline__ void dc_smul(const uint32_t* in, uint32_t* out_wire, size_t row, uint32_t role) {
    Xyzz base;
    dc_smul_base(base, in);
    uint32_t kk[8];
    for (int j = 0; j < 8; ++j) kk[j] = in[32 + j];
    if constexpr (FORM == DC_LANE) {
        Xyzz r;
        uint32_t y[32];
        xyzz_scalar_mul(r, base, kk);
        xyzz_to_wire(y, r);
        for (int j = 0; j < 32; ++j) out_wire[row * 32 + j] = y[j];
    } else if constexpr (FORM == DC_PAIR) {
        const bool odd = role != 0;
        HalfXyzz p, r;
        dc_half_pick(p, base, odd);
        pair_scalar_mul(r, p, kk, odd);
        half_store_wire(out_wire, row, r, odd);
    } else {
        QuadXyzz p, r;
        dc_quad_pick(p, base, role);
        quad_scalar_mul(r, p, kk, role);
        quad_store_wire(out_wire, row, r, role);
    }
}

// The three row semantics of dc_curve (dc_prims.h) through the lane-form formulas:
//   DC_MADD: P1 + (sign ? -P2 : P2) by pair_madd / quad_madd
//   DC_PADD: (P1 + P2) + 2 P2 by pair_add / quad_add (the 2 P2 by pair_dbl / quad_dbl)
//   DC_PDBL: 2 (P1 + P2) by pair_dbl_any / quad_dbl_any (pair_dbl / quad_dbl, and the identity passed through when P1 == -P2)
template <int FORM, int OP>
__device__ __forceinline__ void dc_lanes_curve(const uint32_t* in, uint32_t* out_wire, size_t row, uint32_t role) {
    static_assert(FORM == DC_PAIR || FORM == DC_QUAD, "lane forms only");
    Affine p1, p2;
    const bool has1 = dc_load_point(p1, in);
    dc_load_point(p2, in + 16);
    const uint32_t neg = in[32] & 1u;
    Xyzz a1, b1;
    if (has1) xyzz_from_affine(a1, p1, 0); else xyzz_set_inf(a1);
    xyzz_from_affine(b1, p2, 0);
    if constexpr (FORM == DC_PAIR) {
        const bool odd = role != 0;
        const Fq c = odd ? p2.y : p2.x;
        HalfXyzz a, b, s, t, r;
        dc_half_pick(a, a1, odd);
        if constexpr (OP == DC_MADD) {
            pair_madd(r, a, c, neg, odd);
        } else if constexpr (OP == DC_PADD) {
            pair_madd(s, a, c, 0, odd);
            dc_half_pick(b, b1, odd);
            pair_dbl(t, b, odd);
            pair_add(r, s, t, odd);
        } else {
            pair_madd(s, a, c, 0, odd);
            pair_dbl_any(r, s, odd);
        }
        half_store_wire(out_wire, row, r, odd);
    } else {
        const Fq c = (role & 1u) ? p2.y : p2.x;
        QuadXyzz a, b, s, t, r;
        dc_quad_pick(a, a1, role);
        if constexpr (OP == DC_MADD) {
            quad_madd(r, a, c, neg, role);
        } else if constexpr (OP == DC_PADD) {
            quad_madd(s, a, c, 0, role);
            dc_quad_pick(b, b1, role);
            quad_dbl(t, b, role);
            quad_add(r, s, t, role);
        } else {
            quad_madd(s, a, c, 0, role);
            quad_dbl_any(r, s, role);
        }
        quad_store_wire(out_wire, row, r, role);
    }
}

}  // namespace kzg
