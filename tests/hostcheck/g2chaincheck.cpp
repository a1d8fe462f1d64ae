// tests/hostcheck/g2chaincheck.cpp — TEST-ONLY host build of the per-lane G2 chains (csrc/g2_chain.h) compiled by g++ with
// -DKZG_BOUND_CHECK (every lazy-reduction bound aborts), compared BY VALUE with the independent G2 arithmetic of csrc/host_pairing.h
// (4 x 64-bit Montgomery limbs, affine and Jacobian formulas, the host's own Frobenius constants).  Loaded only by
// tests/test_g2_chain_host.py.  Every entry returns 0 when the two sides agree.
#include <cstdint>
#include <cstring>
#include "g2_chain.h"
#include "host_pairing.h"

using namespace kzg;
namespace H = kzg_host;

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
static bool stored_form(const G2Xyzz& v) { return v.inf || (in_class_f(v.x) && in_class_f(v.y) && in_class_f(v.zz) && in_class_f(v.zzz)); }
static H::G2 host_of_xyzz(const G2Xyzz& v) {
    if (v.inf) return H::g2_inf();
    const H::Fq2 x = host_of_fq2(v.x), y = host_of_fq2(v.y), zz = host_of_fq2(v.zz), zzz = host_of_fq2(v.zzz);
    if (H::is_zero(zz)) return H::g2_inf();
    H::G2 r; r.inf = false;
    r.x = H::mul(x, H::inv(zz));
    r.y = H::mul(y, H::inv(zzz));
    return r;
}
static H::G2 host_of_affine(const G2Affine& p) {
    H::G2 r; r.inf = false;
    r.x = host_of_fq2(p.x); r.y = host_of_fq2(p.y);
    return r;
}
static bool same_point(const H::G2& a, const H::G2& b) {
    if (a.inf || b.inf) return a.inf == b.inf;
    return H::eq(a.x, b.x) && H::eq(a.y, b.y);
}
static bool load_affine(G2Affine& p, const uint32_t* wire32) {
    uint32_t dev[32];
    bool on;
    g2_affine_wire_to_device(dev, wire32, &on);
    uint4 q[8];
    memcpy(q, dev, 128);
    return g2_affine_load(p, q);
}
// [k]P on the host for a scalar of `words` 64-bit words (cofactor multiples are longer than 256 bits)
static H::G2 host_mul_words(const H::G2& p, const uint64_t* k, int words) {
    if (p.inf) return p;
    H::G2Jac acc; acc.inf = true; acc.X = {H::fq_zero(), H::fq_zero()}; acc.Y = acc.X; acc.Z = acc.X;
    for (int i = 64 * words - 1; i >= 0; --i) {
        acc = H::g2j_dbl(acc);
        if ((k[i >> 6] >> (i & 63)) & 1) acc = H::g2j_madd(acc, p);
    }
    if (acc.inf) return H::g2_inf();
    const H::Fq2 zi = H::inv(acc.Z), zi2 = H::sqr(zi);
    H::G2 r; r.inf = false;
    r.x = H::mul(acc.X, zi2);
    r.y = H::mul(acc.Y, H::mul(zi2, zi));
    return r;
}
static const uint64_t FR_MODULUS[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};

extern "C" {

// helpers of the test: [k]G2, [k]P for a long scalar, P + Q, all on the host side
void g2cc_mul_generator(const uint64_t* k4, uint64_t* out16) { H::g2_to_wire(H::g2_mul_generator(k4), out16); }
void g2cc_host_mul(const uint64_t* p16, const uint64_t* k, int words, uint64_t* out16) { H::g2_to_wire(host_mul_words(H::g2_from_wire(p16), k, words), out16); }
void g2cc_host_add(const uint64_t* a16, const uint64_t* b16, uint64_t* out16) { H::g2_to_wire(H::g2_add(H::g2_from_wire(a16), H::g2_from_wire(b16)), out16); }
int g2cc_host_on_twist(const uint64_t* p16) { return H::g2_on_curve(H::g2_from_wire(p16)) ? 1 : 0; }

// the limb constants of g2_psi_constants are the host's TWIST_FROB_* by value
int g2cc_psi_constants() {
    Fq2 gx, gy;
    g2_psi_constants(gx, gy);
    if (!fe_bound_canon(gx.c0) || !fe_bound_canon(gx.c1) || !fe_bound_canon(gy.c0) || !fe_bound_canon(gy.c1)) return 2;
    const H::Fq2 hx = host_of_fq2(gx), hy = host_of_fq2(gy);
    const bool ok = H::eq(hx.c0, H::TWIST_FROB_X0) && H::eq(hx.c1, H::TWIST_FROB_X1) && H::eq(hy.c0, H::TWIST_FROB_Y0) && H::eq(hy.c1, H::TWIST_FROB_Y1);
    return ok ? 0 : 1;
}
// psi and psi^2 of an affine point, on the affine form and on an XYZZ form with ZZ != 1 (the point doubled), against g2_frobenius
int g2cc_psi(const uint32_t* wire32) {
    G2Affine p;
    if (!load_affine(p, wire32)) return 3;
    const H::G2 hp = H::g2_from_wire(reinterpret_cast<const uint64_t*>(wire32));
    const H::G2 h1 = H::g2_frobenius(hp), h2 = H::g2_frobenius(h1);
    G2Affine a = p;
    g2_psi(a);
    if (!same_point(host_of_affine(a), h1)) return 1;
    g2_psi(a);
    if (!same_point(host_of_affine(a), h2)) return 1;
    G2Xyzz v, d;
    g2_from_affine(v, p, 0);
    g2_dbl(d, v);                              // [2]P with ZZ, ZZZ != 1
    const H::G2 hd = H::g2_add(hp, hp), hd1 = H::g2_frobenius(hd), hd2 = H::g2_frobenius(hd1);
    g2_psi_xyzz(d);
    if (!stored_form(d)) return 2;
    if (!same_point(host_of_xyzz(d), hd.inf ? hd : hd1)) return 4;
    g2_psi_xyzz(d);
    if (!stored_form(d)) return 2;
    if (!same_point(host_of_xyzz(d), hd.inf ? hd : hd2)) return 4;
    G2Xyzz inf;
    g2_set_inf(inf);
    g2_psi_xyzz(inf);
    return inf.inf ? 0 : 5;
}
// [x]P against the host's g2_mul with BN_X
int g2cc_mul_x(const uint32_t* wire32) {
    G2Affine p;
    if (!load_affine(p, wire32)) return 3;
    G2Xyzz r;
    g2_mul_x(r, p);
    if (!stored_form(r)) return 2;
    const uint64_t k[4] = {H::BN_X, 0, 0, 0};
    if (((uint64_t)G2_BN_X_HI << 32 | G2_BN_X_LO) != H::BN_X) return 6;
    const H::G2 want = host_mul_words(H::g2_from_wire(reinterpret_cast<const uint64_t*>(wire32)), k, 4);
    return same_point(host_of_xyzz(r), want) ? 0 : 1;
}
// [k mod 2^bits]P against the host
int g2cc_mul_bits(const uint32_t* wire32, const uint32_t* k8, int bits) {
    G2Affine p;
    if (!load_affine(p, wire32)) return 3;
    G2Xyzz r;
    g2_mul_bits(r, p, k8, bits);
    if (!stored_form(r)) return 2;
    uint64_t k[4] = {0, 0, 0, 0};
    for (int b = 0; b < bits; ++b) if ((k8[b >> 5] >> (b & 31)) & 1u) k[b >> 6] |= 1ULL << (b & 63);
    const H::G2 want = host_mul_words(H::g2_from_wire(reinterpret_cast<const uint64_t*>(wire32)), k, 4);
    return same_point(host_of_xyzz(r), want) ? 0 : 1;
}
// g2_in_subgroup against the host's [r]P == O; *out_in = the device header's answer (the identity is in the subgroup: no chain runs)
int g2cc_in_subgroup(const uint32_t* wire32, int* out_in) {
    G2Affine p;
    const H::G2 hp = H::g2_from_wire(reinterpret_cast<const uint64_t*>(wire32));
    const bool want = host_mul_words(hp, FR_MODULUS, 4).inf;
    const bool got = load_affine(p, wire32) ? g2_in_subgroup(p) : true;
    *out_in = got ? 1 : 0;
    return got == want ? 0 : 1;
}

}  // extern "C"
