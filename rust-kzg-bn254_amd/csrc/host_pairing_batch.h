// host_pairing_batch.h — the pure host side of the batched pairing checks (pairing.hip): the argument table of
// kzg_pairings_product_verify_batch / kzg_pairings_product_gt_batch in its order, the launch plan, the host's GT value of one check
// (kzg_pairings_product_gt), and the constant tables of the device pairing, derived from host_pairing.h's own (never typed in).
// Nothing here touches a device: tests/hostcheck/pairingdevcheck.cpp compiles it with g++.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "../../include/kzg_bn254_mi355x.h"
#include "host_pairing.h"
#include "pairing_dev.h"

namespace kzg_host {

// One check is one lane's work from its first pair to its verdict (about 40 000 Fq products for two pairs), so a check may not be
// arbitrarily long, and the staged points of a call are bounded: 2^20 pairs are 192 MiB of wire points.
constexpr size_t PAIRING_BATCH_MAX_CHECKS = (size_t)1 << 20;
constexpr size_t PAIRING_BATCH_MAX_PAIRS = (size_t)1 << 20;
constexpr size_t PAIRING_BATCH_MAX_PAIRS_PER_CHECK = 64;
constexpr unsigned PAIRING_BLOCK = 64;         // one wave per workgroup: a check per lane

// The argument table, decided before the context is dereferenced (ctx is only compared with null).  *total = pair_offsets[n_checks].
inline int32_t pairing_batch_check_args(const void* ctx, const uint64_t* g1s_xy, const uint64_t* g2s, const uint64_t* pair_offsets, size_t n_checks,
                                        const void* out, size_t* total) {
    *total = 0;
    if (!ctx || !pair_offsets || (n_checks && !out)) return KZG_ERR_INVALID_ARG;
    if (n_checks > PAIRING_BATCH_MAX_CHECKS) return KZG_ERR_TOO_LARGE;
    if (pair_offsets[0] != 0) return KZG_ERR_INVALID_ARG;
    for (size_t i = 0; i < n_checks; ++i)
        if (pair_offsets[i + 1] < pair_offsets[i]) return KZG_ERR_INVALID_ARG;
    for (size_t i = 0; i < n_checks; ++i)
        if (pair_offsets[i + 1] - pair_offsets[i] > PAIRING_BATCH_MAX_PAIRS_PER_CHECK) return KZG_ERR_TOO_LARGE;
    if (pair_offsets[n_checks] > PAIRING_BATCH_MAX_PAIRS) return KZG_ERR_TOO_LARGE;
    if (pair_offsets[n_checks] && (!g1s_xy || !g2s)) return KZG_ERR_INVALID_ARG;
    *total = (size_t)pair_offsets[n_checks];
    return KZG_OK;
}

// Where a call's arrays lie in its three device buffers (bytes) and how many workgroups its two kernels take
struct PairingBatchPlan {
    size_t n_checks = 0, total = 0;
    size_t wire_g1 = 0, wire_g2 = 0, wire_bytes = 0;                          // buffer 0: the wire points as uploaded
    size_t dev_g1 = 0, dev_g2 = 0, dev_offsets = 0, dev_flags = 0, dev_bytes = 0;   // buffer 1: device-format points, the offsets (u32), a flag byte per pair
    size_t out_gt = 0, out_ok = 0, out_bytes = 0;                             // buffer 2: 96 u32 per check, a verdict byte per check
    unsigned convert_blocks = 0, check_blocks = 0;
};
inline PairingBatchPlan pairing_batch_plan(size_t n_checks, size_t total) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    PairingBatchPlan p;
    p.n_checks = n_checks; p.total = total;
    p.wire_g1 = 0; p.wire_g2 = up(total * 64); p.wire_bytes = p.wire_g2 + up(total * 128);
    p.dev_g1 = 0; p.dev_g2 = up(total * 64); p.dev_offsets = p.dev_g2 + up(total * 128); p.dev_flags = p.dev_offsets + up((n_checks + 1) * 4);
    p.dev_bytes = p.dev_flags + up(total);
    p.out_gt = 0; p.out_ok = up(n_checks * 384); p.out_bytes = p.out_ok + up(n_checks);
    p.convert_blocks = (unsigned)((total + 255) / 256);
    p.check_blocks = (unsigned)((n_checks + PAIRING_BLOCK - 1) / PAIRING_BLOCK);
    return p;
}

// The GT value of prod_k e(ps[k], qs[k]) as the host computes it: chunks as in pairings_product_is_one, ONE final exponentiation.
// false: an addition step was degenerate (a G2 point outside the order-r subgroup): there is no value, *out is zero.
inline bool pairings_product_gt(const G1* ps, const G2* qs, int count, Fq12* out, PairingParallelFor parallel_for = nullptr) {
    std::vector<G1> p1;
    std::vector<G2> q2;
    for (int k = 0; k < count; ++k) {
        if (ps[k].inf || qs[k].inf) continue;
        p1.push_back(ps[k]); q2.push_back(qs[k]);
    }
    const size_t m = p1.size();
    if (m == 0) { *out = fq12_one(); return true; }
    const size_t per = parallel_for && m > 1 ? 1 : 4, chunks = (m + per - 1) / per;
    std::vector<Fq12> f(chunks);
    std::vector<uint8_t> bad(chunks, 0);
    auto body = [&](size_t c) {
        bool d = false;
        const size_t lo = c * per, len = m - lo < per ? m - lo : per;
        f[c] = miller_ate_product(p1.data() + lo, q2.data() + lo, (int)len, &d);
        bad[c] = d ? 1 : 0;
    };
    if (parallel_for && chunks > 1) parallel_for(chunks, body);
    else for (size_t c = 0; c < chunks; ++c) body(c);
    Fq12 prod = f[0];
    for (size_t c = 0; c < chunks; ++c) {
        if (bad[c]) { memset(out, 0, sizeof *out); return false; }
        if (c) prod = mul(prod, f[c]);
    }
    *out = final_exponentiation_x(prod);
    return true;
}

// ---- the device pairing's constants from the host's tables --------------------------------------------------------------------
inline void pairing_pack_fq(uint32_t out[8], const Fq& a) {          // wire words -> canonical residue of the internal form
    uint32_t w[8];
    memcpy(w, a.l, 32);
    kzg::Fq t;
    kzg::fe_from_wire(t, w);
    kzg::fe_canon(t);
    kzg::fe_pack(out, t);
}
// false: a table of host_pairing.h does not have the shape the device form relies on ((w^i)^(p^k) = gamma w^i with gamma in Fq2)
inline bool pairing_consts_build(kzg::PairingConsts* out) {
    memset(out, 0, sizeof *out);
    const FrobeniusTables& t = frobenius_tables();
    for (int k = 0; k < 3; ++k)
        for (int i = 1; i < 6; ++i) {
            const Fq12& e = t.w[k][i];
            for (int j = 0; j < 12; ++j)
                if (j != i && j != i + 6 && !is_zero(e.c[j])) return false;
            // gamma = c_i + c_(i+6) w^6 = (c_i + 9 c_(i+6)) + c_(i+6) u
            const Fq c0 = add(e.c[i], mul(e.c[i + 6], FQ_NINE));
            pairing_pack_fq(out->frob[k][i - 1], c0);
            pairing_pack_fq(out->frob[k][i - 1] + 8, e.c[i + 6]);
        }
    pairing_pack_fq(out->twist_frob_x, TWIST_FROB_X0); pairing_pack_fq(out->twist_frob_x + 8, TWIST_FROB_X1);
    pairing_pack_fq(out->twist_frob_y, TWIST_FROB_Y0); pairing_pack_fq(out->twist_frob_y + 8, TWIST_FROB_Y1);
    pairing_pack_fq(out->twist_frob2_x, TWIST_FROB2_X);
    const AteNaf& naf = ate_naf();
    if (naf.len < 2 || naf.len > 66) return false;
    out->naf_len = naf.len;
    for (int i = 0; i < naf.len; ++i) out->naf[i] = naf.d[i];
    return true;
}

}  // namespace kzg_host
