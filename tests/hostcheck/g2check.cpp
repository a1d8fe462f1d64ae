// tests/hostcheck/g2check.cpp — TEST-ONLY host build of the device G2 math (csrc/fq2.h, csrc/curve_g2.h) compiled by g++ with
// -DKZG_BOUND_CHECK (every lazy-reduction bound aborts), compared BY VALUE with the independent Fq2 / G2 arithmetic of
// csrc/host_pairing.h (4 x 64-bit Montgomery limbs, affine and Jacobian formulas).  Loaded only by tests/test_g2_math_host.py.
// Every entry returns 0 when the two sides agree.
#include <cstdint>
#include <cstring>
#include <vector>
#include "curve_g2.h"
#include "host_pairing.h"

using namespace kzg;
namespace H = kzg_host;

// raw signed limbs (value v = sum l_j 2^(29 j), any lazy representative with |v| < 169 m) -> the host's element of the same residue
static H::Fq host_of_limbs(const int32_t* l) {
    Fq a;
    for (int j = 0; j < NL; ++j) a.l[j] = l[j];
    fe_reduce(a);
    uint32_t w[8];
    fe_to_wire(w, a);
    H::Fq r;
    memcpy(r.l, w, 32);
    return r;
}
static H::Fq2 host_of_fq2(const Fq2& a) {
    Fq2 t = a;
    fq2_norm(t);
    uint32_t w[16];
    fq2_to_wire(w, t);
    H::Fq2 r;
    memcpy(r.c0.l, w, 32); memcpy(r.c1.l, w + 8, 32);
    return r;
}
static bool in_class_f(const Fq2& a) { return fe_bound_canon(a.c0) && fe_bound_canon(a.c1); }

// device XYZZ -> host affine point through the wire form (x = X / ZZ, y = Y / ZZZ with the host's inversion)
static H::G2 host_of_xyzz(const G2Xyzz& v) {
    uint32_t w[64];
    g2_to_wire(w, v);
    H::Fq2 c[4];
    for (int q = 0; q < 4; ++q) { memcpy(c[q].c0.l, w + 16 * q, 32); memcpy(c[q].c1.l, w + 16 * q + 8, 32); }
    if (v.inf || H::is_zero(c[2])) return H::g2_inf();
    H::G2 r; r.inf = false;
    r.x = H::mul(c[0], H::inv(c[2]));
    r.y = H::mul(c[1], H::inv(c[3]));
    return r;
}
static bool same_point(const H::G2& a, const H::G2& b) {
    if (a.inf || b.inf) return a.inf == b.inf;
    return H::eq(a.x, b.x) && H::eq(a.y, b.y);
}
static bool stored_form(const G2Xyzz& v) { return v.inf || (in_class_f(v.x) && in_class_f(v.y) && in_class_f(v.zz) && in_class_f(v.zzz)); }
static bool load_affine(G2Affine& p, const uint32_t* wire32) {
    uint32_t dev[32];
    bool on;
    g2_affine_wire_to_device(dev, wire32, &on);
    uint4 q[8];
    memcpy(q, dev, 128);
    return g2_affine_load(p, q);
}

extern "C" {

// a, b: 18 raw limbs each (c0 | c1).  op 0: fq2_mul, 1: fq2_sqr(a), 2: fq2_mul_lazy (unreduced), 3: fq2_mul_fq(a, b.c0)
int g2c_product_vs_host(const int32_t* a18, const int32_t* b18, int op) {
    Fq2 a, b, r;
    for (int j = 0; j < NL; ++j) { a.c0.l[j] = a18[j]; a.c1.l[j] = a18[NL + j]; b.c0.l[j] = b18[j]; b.c1.l[j] = b18[NL + j]; }
    const H::Fq2 ha = {host_of_limbs(a18), host_of_limbs(a18 + NL)}, hb = {host_of_limbs(b18), host_of_limbs(b18 + NL)};
    H::Fq2 want;
    // the device values carry the radix 2^261 and the host's 2^256: a b R'^-1 on one side is a b R^-1 on the other once both are wire
    if (op == 0) { fq2_mul(r, a, b); want = H::mul(ha, hb); }
    else if (op == 1) { fq2_sqr(r, a); want = H::sqr(ha); }
    else if (op == 2) { fq2_mul_lazy(r, a, b); want = H::mul(ha, hb); }
    else { fq2_mul_fq(r, a, b.c0); want = H::mul_fq(ha, hb.c0); }
    if (op != 2 && !in_class_f(r)) return 2;
    // wire(x) = x 2^256, internal(x) = x 2^261: the raw limbs above are INTERNAL values, host_of_limbs made them wire, and the product
    // of two internal values is internal again, so both sides are the wire form of the same residue
    return H::eq(host_of_fq2(r), want) ? 0 : 1;
}
// 1 / a for a wire element (16 u32); 0 -> 0
int g2c_inverse_vs_host(const uint32_t* a16) {
    Fq2 a, r;
    fq2_from_wire(a, a16);
    fq2_inv(r, a);
    H::Fq2 ha;
    memcpy(ha.c0.l, a16, 32); memcpy(ha.c1.l, a16 + 8, 32);
    const H::Fq2 want = H::is_zero(ha) ? ha : H::inv(ha);
    return in_class_f(r) && H::eq(host_of_fq2(r), want) ? 0 : 1;
}
// [k] G2 for canonical integer words k (the host's fixed-base tables): wire affine point
void g2c_mul_generator(const uint64_t* k4, uint64_t* out16) { H::g2_to_wire(H::g2_mul_generator(k4), out16); }

// acc = sum (+-) p_i by the checked mixed addition in the order given (identity bases skipped as the kernels skip them); the stored
// form is asserted after every step.  Compared with the host's Jacobian chain.
int g2c_madd_chain_vs_host(const uint32_t* wire, const uint8_t* signs, size_t n, int inline_slow) {
    G2Xyzz acc;
    g2_set_inf(acc);
    H::G2Jac ref; ref.inf = true; ref.X = {H::fq_zero(), H::fq_zero()}; ref.Y = ref.X; ref.Z = ref.X;
    for (size_t i = 0; i < n; ++i) {
        G2Affine p;
        H::G2 hp = H::g2_from_wire(reinterpret_cast<const uint64_t*>(wire + 32 * i));
        if (!load_affine(p, wire + 32 * i)) { if (!hp.inf) return 3; continue; }
        if (inline_slow) g2_madd<true>(acc, p, signs[i]); else g2_madd<false>(acc, p, signs[i]);
        if (!stored_form(acc)) return 2;
        ref = H::g2j_madd(ref, signs[i] ? H::g2_neg(hp) : hp);
    }
    H::G2 want = H::g2_inf();
    if (!ref.inf) {
        const H::Fq2 zi = H::inv(ref.Z), zi2 = H::sqr(zi);
        want.inf = false; want.x = H::mul(ref.X, zi2); want.y = H::mul(ref.Y, H::mul(zi2, zi));
    }
    return same_point(host_of_xyzz(acc), want) ? 0 : 1;
}
// (sum of the first half) + (sum of the second half) by the FULL addition, both halves stored to and loaded from the 72-plane memory
// form first, then `dbl` doublings of the stored value; compared with the host's affine additions
int g2c_add_halves_vs_host(const uint32_t* wire, const uint8_t* signs, size_t n, int dbl) {
    G2Xyzz half[2];
    H::G2 want = H::g2_inf();
    for (int h = 0; h < 2; ++h) {
        g2_set_inf(half[h]);
        const size_t lo = h ? n / 2 : 0, hi = h ? n : n / 2;
        for (size_t i = lo; i < hi; ++i) {
            G2Affine p;
            if (!load_affine(p, wire + 32 * i)) continue;
            g2_madd(half[h], p, signs[i]);
            const H::G2 hp = H::g2_from_wire(reinterpret_cast<const uint64_t*>(wire + 32 * i));
            want = H::g2_add(want, signs[i] ? H::g2_neg(hp) : hp);
        }
    }
    std::vector<int32_t> mem((size_t)G2_LIMBS * 3, 0x5a5a5a5a);
    g2_store(mem.data(), 3, 0, half[0]);
    g2_store(mem.data(), 3, 2, half[1]);
    G2Xyzz a, b, r;
    g2_load(a, mem.data(), 3, 0);
    g2_load(b, mem.data(), 3, 2);
    if (a.inf != half[0].inf || b.inf != half[1].inf) return 4;
    g2_add(r, a, b);
    if (!stored_form(r)) return 2;
    for (int k = 0; k < dbl; ++k) {
        G2Xyzz d;
        g2_dbl(d, r);
        r = d;
        if (!stored_form(r)) return 2;
        want = H::g2_add(want, want);
    }
    if (!same_point(host_of_xyzz(r), want)) return 1;
    // the affine conversion of the device header (one Fq2 inversion)
    if (!r.inf) {
        Fq2 x, y;
        g2_to_affine(x, y, r);
        if (!H::eq(host_of_fq2(x), want.x) || !H::eq(host_of_fq2(y), want.y)) return 5;
    }
    return 0;
}
// r = a + b for two AFFINE wire points taken to XYZZ first; which = 0: full add, 1: mixed add of b onto a, 2: a + a by g2_dbl.
// Covers the operand positions of the exceptional cases.
int g2c_pair_vs_host(const uint32_t* a32, const uint32_t* b32, int which) {
    G2Affine pa, pb;
    const bool fa = load_affine(pa, a32), fb = load_affine(pb, b32);
    G2Xyzz xa, xb, r;
    if (fa) g2_from_affine(xa, pa, 0); else g2_set_inf(xa);
    if (fb) g2_from_affine(xb, pb, 0); else g2_set_inf(xb);
    const H::G2 ha = H::g2_from_wire(reinterpret_cast<const uint64_t*>(a32)), hb = H::g2_from_wire(reinterpret_cast<const uint64_t*>(b32));
    H::G2 want;
    if (which == 0) { g2_add(r, xa, xb); want = H::g2_add(ha, hb); }
    else if (which == 1) { r = xa; if (fb) g2_madd(r, pb, 0); want = H::g2_add(ha, hb); }
    else { g2_dbl(r, xa); want = H::g2_add(ha, ha); }
    if (!stored_form(r)) return 2;
    return same_point(host_of_xyzz(r), want) ? 0 : 1;
}
// wire -> device format -> wire is the identity map; *on_twist as the host's g2_on_curve says
int g2c_wire_roundtrip(const uint32_t* in32) {
    uint32_t dev[32], back[32];
    bool on;
    g2_affine_wire_to_device(dev, in32, &on);
    g2_affine_device_to_wire(back, dev);
    if (memcmp(back, in32, 128) != 0) return 1;
    const H::G2 hp = H::g2_from_wire(reinterpret_cast<const uint64_t*>(in32));
    return on == H::g2_on_curve(hp) ? 0 : 6;
}
// the generator constant of curve_g2.h is the host's
int g2c_generator_matches() {
    uint32_t w[32];
    g2_generator_wire(w);
    uint64_t h[16];
    H::g2_to_wire(H::g2_generator(), h);
    return memcmp(w, h, 128) == 0 ? 0 : 1;
}

}  // extern "C"
