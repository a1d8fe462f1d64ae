// tests/hostcheck/pairingdevcheck.cpp — TEST-ONLY host build of the device pairing (csrc/fq12.h, csrc/pairing_dev.h) and of the pure host side of
// the batched entries (csrc/host_pairing_batch.h), compiled by g++ with -DKZG_BOUND_CHECK (every lazy-reduction bound aborts) and compared BY
// VALUE with csrc/host_pairing.h, the oracle: other limb size, the flat form of Fq12, other product formulas.
// A stand-alone program (tests/test_pairing_device_host.py runs it once as it is and once under ASan + UBSan).
//   argv[1]  a file of int32 limbs, 9 per Fq operand (the extreme limb patterns of tests/fe_operands.py), or "-"
//   argv[2]  96 hex words: the two (G1, G2) pairs of the EIP-197 known answer as wire words, e(P1, Q1) e(P2, Q2) == 1
// Prints "pairingdevcheck ok" and returns 0 when every comparison holds; otherwise the first failure and 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "curve_g2.h"
#include "host_pairing_batch.h"

using namespace kzg;
namespace H = kzg_host;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "pairingdevcheck FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

static uint64_t g_seed = 88172645463325252ULL;
static uint64_t rnd64() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }
static H::Fq rnd_fq() {
    H::Fq t = {{rnd64(), rnd64(), rnd64(), rnd64()}};
    t.l[3] &= (1ULL << 61) - 1;                    // < 2^253 < p: any such words are a wire value
    return t;
}
static H::Fq12 rnd_fq12() { H::Fq12 r; for (int i = 0; i < 12; ++i) r.c[i] = rnd_fq(); return r; }
static void rnd_scalar(uint64_t k[4]) { for (int i = 0; i < 4; ++i) k[i] = rnd64(); k[3] &= (1ULL << 60) - 1; }

static bool host_eq(const H::Fq12& a, const H::Fq12& b) { for (int i = 0; i < 12; ++i) if (!H::eq(a.c[i], b.c[i])) return false; return true; }
static Fq12 dev_of(const H::Fq12& a) {
    uint32_t w[96];
    memcpy(w, a.c, 384);
    Fq12 r;
    fq12_from_flat_wire(r, w);
    return r;
}
static H::Fq12 host_of(const Fq12& a) {
    uint32_t w[96];
    fq12_to_flat_wire(w, a);
    H::Fq12 r;
    memcpy(r.c, w, 384);
    return r;
}
static bool stored_form(const Fq12& a) {           // every component normalised and inside class O: (-0.0001m, 1.0001m)
    for (int i = 0; i < 6; ++i)
        for (const Fq* c : {&a.g[i].c0, &a.g[i].c1}) {
            if (!fe_bound_normalised(*c)) return false;
            const double v = fe_value_approx(*c) / fe_modulus_approx<FqParams>();
            if (v <= -0.0001 || v >= 1.0001) return false;
        }
    return true;
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
static Fq2 dev_of_fq2(const H::Fq2& a) {
    uint32_t w[16];
    memcpy(w, a.c0.l, 32); memcpy(w + 8, a.c1.l, 32);
    Fq2 r;
    fq2_from_wire(r, w);
    fq2_reduce(r);
    return r;
}
static H::Fq host_of_packed(const uint32_t p[8]) {
    Fq t;
    fe_unpack(t, p);
    uint32_t w[8];
    fe_to_wire(w, t);
    H::Fq r;
    memcpy(r.l, w, 32);
    return r;
}

static PairingConsts g_consts;

// every Fq12 operation on one pair of operands (device stored form on one side, the host's flat form on the other)
static int ops_by_value(const Fq12& a, const Fq12& b, const char* what) {
    const H::Fq12 ha = host_of(a), hb = host_of(b);
    Fq12 r;
    fq12_mul(r, a, b);
    CHECK(stored_form(r) && host_eq(host_of(r), H::mul(ha, hb)), "fq12_mul (%s)", what);
    fq12_sqr(r, a);
    CHECK(stored_form(r) && host_eq(host_of(r), H::sqr(ha)), "fq12_sqr (%s)", what);
    { Fq12 x = a; fq12_mul(x, x, x); CHECK(host_eq(host_of(x), H::sqr(ha)), "fq12_mul in place (%s)", what); }
    fq12_conj(r, a);
    CHECK(stored_form(r) && host_eq(host_of(r), H::conjugate_p6(ha)), "fq12_conj (%s)", what);
    for (int k = 1; k <= 3; ++k) {
        fq12_frobenius(r, a, k, g_consts);
        CHECK(stored_form(r) && host_eq(host_of(r), H::frobenius(ha, k)), "fq12_frobenius %d (%s)", k, what);
    }
    fq12_cyclotomic_sqr(r, a);                      // the same formula on both sides, whatever the operand: the square only inside the subgroup
    CHECK(stored_form(r) && host_eq(host_of(r), H::cyclotomic_sqr(ha)), "fq12_cyclotomic_sqr (%s)", what);
    {   // line product: a line from three coefficients of b
        AteLine l = {b.g[0], b.g[1], b.g[2]};
        H::AteLine hl = {host_of_fq2(b.g[0]), host_of_fq2(b.g[1]), host_of_fq2(b.g[2])};
        r = a;
        fq12_mul_by_line(r, l);
        CHECK(stored_form(r) && host_eq(host_of(r), H::mul_by_line(ha, hl)), "fq12_mul_by_line (%s)", what);
    }
    {
        H::Fq12 hi;
        const bool hok = H::fq12_inverse_norm(ha, hi);
        const bool dok = fq12_inverse(r, a, g_consts);
        CHECK(hok == dok, "fq12_inverse: invertible (%s)", what);
        if (hok) CHECK(stored_form(r) && host_eq(host_of(r), hi), "fq12_inverse (%s)", what);
    }
    return 0;
}

static H::G1 g1_gen() { H::G1 g; g.x = H::FQ_ONE; g.y = H::FQ_TWO; g.inf = false; return g; }

// the pairs as the two device-format arrays of pairing_check_dev
static int to_device(const std::vector<H::G1>& ps, const std::vector<H::G2>& qs, std::vector<uint32_t>* g1d, std::vector<uint32_t>* g2d) {
    g1d->assign(16 * ps.size() + 16, 0); g2d->assign(32 * ps.size() + 32, 0);
    for (size_t k = 0; k < ps.size(); ++k) {
        uint64_t a[8], b[16];
        H::g1_to_wire(ps[k], a); H::g2_to_wire(qs[k], b);
        uint32_t aw[16], bw[32];
        memcpy(aw, a, 64); memcpy(bw, b, 128);
        CHECK(pairing_pair_to_device(g1d->data() + 16 * k, g2d->data() + 32 * k, aw, bw) == 0, "pair %zu is refused", k);
    }
    return 0;
}
// device check of the pairs against the host's GT value and verdict
static int check_vs_host(const std::vector<H::G1>& ps, const std::vector<H::G2>& qs, const char* what, int want_verdict = -1) {
    std::vector<uint32_t> g1d, g2d;
    if (to_device(ps, qs, &g1d, &g2d)) return 1;
    uint32_t gt[96];
    const bool ok = pairing_check_dev(gt, g1d.data(), g2d.data(), 0, (uint32_t)ps.size(), g_consts);
    H::Fq12 want;
    const bool have = H::pairings_product_gt(ps.data(), qs.data(), (int)ps.size(), &want);
    CHECK(memcmp(gt, want.c, 384) == 0, "GT words differ from the host's (%s, %zu pairs)", what, ps.size());
    const bool host_ok = H::pairings_product_is_one(ps.data(), qs.data(), (int)ps.size());
    CHECK(ok == host_ok && (have || !ok), "verdict differs from the host's (%s, %zu pairs)", what, ps.size());
    if (want_verdict >= 0) CHECK((int)ok == want_verdict, "verdict %d, expected %d (%s)", (int)ok, want_verdict, what);
    return 0;
}

int main(int argc, char** argv) {
    CHECK(H::pairing_consts_build(&g_consts), "pairing_consts_build: a host table has another shape");
    {   // the tables against the host's, value by value
        const H::FrobeniusTables& t = H::frobenius_tables();
        for (int k = 0; k < 3; ++k)
            for (int i = 1; i < 6; ++i) {
                const H::Fq c1 = host_of_packed(g_consts.frob[k][i - 1] + 8), c0 = host_of_packed(g_consts.frob[k][i - 1]);
                CHECK(H::eq(c1, t.w[k][i].c[i + 6]) && H::eq(H::sub(c0, H::mul(c1, H::FQ_NINE)), t.w[k][i].c[i]), "frobenius table %d %d", k, i);
            }
        CHECK(H::eq(host_of_packed(g_consts.twist_frob_x), H::TWIST_FROB_X0) && H::eq(host_of_packed(g_consts.twist_frob_x + 8), H::TWIST_FROB_X1), "twist_frob_x");
        CHECK(H::eq(host_of_packed(g_consts.twist_frob_y), H::TWIST_FROB_Y0) && H::eq(host_of_packed(g_consts.twist_frob_y + 8), H::TWIST_FROB_Y1), "twist_frob_y");
        CHECK(H::eq(host_of_packed(g_consts.twist_frob2_x), H::TWIST_FROB2_X), "twist_frob2_x");
        const H::AteNaf& naf = H::ate_naf();
        CHECK(g_consts.naf_len == naf.len, "naf length");
        unsigned __int128 s = 0;
        for (int i = naf.len - 1; i >= 0; --i) { CHECK(g_consts.naf[i] == naf.d[i], "naf digit %d", i); s = s * 2 + (unsigned __int128)(__int128)g_consts.naf[i]; }
        CHECK(s == (unsigned __int128)H::BN_X * 6 + 2, "the digits do not sum to 6x + 2");
    }
    // ---- Fq12 operations: random operands, then the operands of the file (extreme limb patterns) ----------------------------------------
    for (int it = 0; it < 24; ++it)
        if (ops_by_value(dev_of(rnd_fq12()), dev_of(rnd_fq12()), "random")) return 1;
    {
        Fq12 one, zero;
        fq12_set_one(one);
        for (int i = 0; i < 6; ++i) fq2_set_zero(zero.g[i]);
        const Fq12 x = dev_of(rnd_fq12());
        if (ops_by_value(one, x, "one") || ops_by_value(x, one, "by one") || ops_by_value(zero, x, "zero") || ops_by_value(x, zero, "by zero")) return 1;
        Fq12 sparse = zero;                          // one coefficient only, at every position
        for (int i = 0; i < 6; ++i) { sparse = zero; sparse.g[i] = x.g[i]; if (ops_by_value(sparse, x, "sparse") || ops_by_value(x, sparse, "by sparse")) return 1; }
    }
    if (argc > 1 && strcmp(argv[1], "-") != 0) {
        FILE* fp = fopen(argv[1], "rb");
        CHECK(fp, "cannot open %s", argv[1]);
        std::vector<Fq> ops;
        int32_t l[NL];
        while (fread(l, 4, NL, fp) == (size_t)NL) {
            // An operand of these functions is a NORMALISED component in class F, (-m, 2m): the pattern's own limbs where its value lies
            // there once the carries are propagated, otherwise its reduced representative (what a stored component of that residue is).
            Fq a;
            for (int j = 0; j < NL; ++j) a.l[j] = l[j];
            fe_norm(a);
            if (!fe_bound_canon(a)) fe_reduce_small(a);
            ops.push_back(a);
        }
        fclose(fp);
        CHECK(ops.size() >= 24, "the operand file holds %zu operands", ops.size());
        for (size_t s = 0; s < ops.size(); ++s) {
            Fq12 a, b;
            for (int i = 0; i < 6; ++i) {
                a.g[i].c0 = ops[(s + 5 * i) % ops.size()]; a.g[i].c1 = ops[(s * 3 + 7 * i + 1) % ops.size()];
                b.g[i].c0 = ops[(s * 7 + 11 * i + 2) % ops.size()]; b.g[i].c1 = ops[(s + 13 * i + 3) % ops.size()];
            }
            if (ops_by_value(a, b, "extreme limb patterns")) return 1;
            Fq12 same;                               // the same pattern in all twelve components
            for (int i = 0; i < 6; ++i) { same.g[i].c0 = ops[s]; same.g[i].c1 = ops[s]; }
            if (ops_by_value(same, same, "one pattern everywhere")) return 1;
        }
    }
    // ---- points ---------------------------------------------------------------------------------------------------------------------------
    const H::G1 g1 = g1_gen();
    const H::G2 g2 = H::g2_generator();
    std::vector<H::G1> P;
    std::vector<H::G2> Q;
    for (int k = 0; k < 5; ++k) {
        uint64_t a[4], b[4];
        rnd_scalar(a); rnd_scalar(b);
        P.push_back(H::g1_mul(g1, a)); Q.push_back(H::g2_mul(g2, b));
    }
    {   // cyclotomic squaring and the power by x on members of the subgroup
        const H::Fq12 e = H::pairing_ate(P[0], Q[0]);
        Fq12 r;
        fq12_cyclotomic_sqr(r, dev_of(e));
        CHECK(host_eq(host_of(r), H::sqr(e)), "cyclotomic square of a GT element is not its square");
        fq12_pow_x(r, dev_of(e));
        CHECK(stored_form(r) && host_eq(host_of(r), H::fq12_pow_x(e)), "fq12_pow_x");
        const H::Fq12 m = H::miller_ate_product(&P[1], &Q[1], 1);
        fq12_final_exponentiation(r, dev_of(m), g_consts);
        CHECK(stored_form(r) && host_eq(host_of(r), H::final_exponentiation_x(m)), "fq12_final_exponentiation");
    }
    {   // both line steps along a whole loop, the two Frobenius steps included: lines and T by value at every step
        const H::G1 p = P[2];
        const H::G2 q = Q[2], nq = H::g2_neg(q);
        H::G2Jac T; T.X = q.x; T.Y = q.y; T.Z = {H::FQ_ONE, H::fq_zero()}; T.inf = false;
        AtePair s;
        {
            uint32_t w[16];
            memcpy(w, p.x.l, 32); memcpy(w + 8, p.y.l, 32);
            Fq px, py;
            fe_from_wire(px, w); fe_from_wire(py, w + 8);
            ate_pair_init(s, px, py, dev_of_fq2(q.x), dev_of_fq2(q.y));
        }
        auto same = [&](const AteLine& l, const H::AteLine& hl) {
            return H::eq(host_of_fq2(l.a), hl.a) && H::eq(host_of_fq2(l.b), hl.b) && H::eq(host_of_fq2(l.c), hl.c) && H::eq(host_of_fq2(s.X), T.X) &&
                   H::eq(host_of_fq2(s.Y), T.Y) && H::eq(host_of_fq2(s.Z), T.Z);
        };
        const H::AteNaf& naf = H::ate_naf();
        AteLine l;
        H::AteLine hl;
        int steps = 0;
        for (int i = naf.len - 2; i >= 0; --i) {
            H::ate_dbl_step(T, p, hl); ate_dbl_step(s, l);
            CHECK(same(l, hl), "doubling step at digit %d", i);
            ++steps;
            if (naf.d[i]) {
                const H::G2& a = naf.d[i] > 0 ? q : nq;
                CHECK(H::ate_add_step(T, a, p, hl), "host addition step degenerate");
                CHECK(ate_add_step(s, dev_of_fq2(a.x), dev_of_fq2(a.y), l), "addition step degenerate at digit %d", i);
                CHECK(same(l, hl), "addition step at digit %d", i);
                ++steps;
            }
        }
        Fq2 x1, y1, x2;
        ate_frobenius_points(x1, y1, x2, s.qx, s.qy, g_consts);
        const H::G2 f1 = H::g2_frobenius(q), f2 = H::g2_frobenius2_neg(q);
        CHECK(H::eq(host_of_fq2(x1), f1.x) && H::eq(host_of_fq2(y1), f1.y) && H::eq(host_of_fq2(x2), f2.x), "Frobenius points");
        CHECK(H::ate_add_step(T, f1, p, hl) && ate_add_step(s, x1, y1, l) && same(l, hl), "first Frobenius step");
        CHECK(H::ate_add_step(T, f2, p, hl) && ate_add_step(s, x2, s.qy, l) && same(l, hl), "second Frobenius step");
        CHECK(steps > 80, "the loop took %d steps", steps);
        // T == Q: the degenerate addition is reported and changes nothing
        AtePair d;
        ate_pair_init(d, s.py, s.py, s.qx, s.qy);
        const AtePair before = d;
        CHECK(!ate_add_step(d, d.qx, d.qy, l) && memcmp(&before, &d, sizeof d) == 0, "T == Q is not reported as degenerate");
    }
    // ---- whole Miller products and checks: 1, 2, 4 and 5 pairs --------------------------------------------------------------------------------
    for (int count : {1, 2, 4}) {
        std::vector<uint32_t> g1d, g2d;
        std::vector<H::G1> ps(P.begin(), P.begin() + count);
        std::vector<H::G2> qs(Q.begin(), Q.begin() + count);
        if (to_device(ps, qs, &g1d, &g2d)) return 1;
        AtePair pts[ATE_CHUNK];
        for (int k = 0; k < count; ++k) {
            Fq px, py;
            Fq2 qx, qy;
            fe_unpack(px, g1d.data() + 16 * k); fe_unpack(py, g1d.data() + 16 * k + 8);
            fq2_unpack(qx, g2d.data() + 32 * k); fq2_unpack(qy, g2d.data() + 32 * k + 16);
            ate_pair_init(pts[k], px, py, qx, qy);
        }
        Fq12 f;
        bool bad = false;
        miller_ate_product_dev(f, pts, count, g_consts, &bad);
        CHECK(!bad && stored_form(f) && host_eq(host_of(f), H::miller_ate_product(ps.data(), qs.data(), count)), "Miller product of %d pairs", count);
    }
    for (int count : {0, 1, 2, 4, 5}) {
        std::vector<H::G1> ps(P.begin(), P.begin() + count);
        std::vector<H::G2> qs(Q.begin(), Q.begin() + count);
        if (check_vs_host(ps, qs, "random pairs", count == 0 ? 1 : 0)) return 1;
    }
    {   // bilinearity: e([a]P, [b]Q) e(-[ab]P, Q) == 1, and not with another scalar
        uint64_t a[4], b[4];
        rnd_scalar(a); rnd_scalar(b);
        uint64_t aw[4], abc[4];
        H::fr_mul(a, H::FR_R2, aw);                 // a in wire form (a < 2^252 < r is canonical)
        H::fr_mul(aw, b, abc);                      // a 2^256 b 2^-256 = a b mod r, canonical words
        const H::G1 pa = H::g1_mul(P[3], a), pab = H::g1_neg(H::g1_mul(P[3], abc));
        const H::G2 qb = H::g2_mul(Q[3], b);
        if (check_vs_host({pa, pab}, {qb, Q[3]}, "bilinear", 1)) return 1;
        if (check_vs_host({pa, pab}, {qb, Q[4]}, "not bilinear", 0)) return 1;
        // identity points in the first, middle and last position contribute 1; five pairs cross the chunk of four
        H::G1 o1; o1.x = H::fq_zero(); o1.y = H::fq_zero(); o1.inf = true;
        if (check_vs_host({o1, pa, pab}, {Q[0], qb, Q[3]}, "identity first", 1)) return 1;
        if (check_vs_host({pa, P[1], pab}, {qb, H::g2_inf(), Q[3]}, "identity middle", 1)) return 1;
        if (check_vs_host({pa, pab, o1}, {qb, Q[3], H::g2_inf()}, "identity last", 1)) return 1;
        if (check_vs_host({pa, P[0], H::g1_neg(P[0]), P[1], H::g1_neg(P[1]), pab}, {qb, Q[0], Q[0], Q[2], Q[2], Q[3]}, "six pairs", 1)) return 1;
        if (check_vs_host({o1, o1}, {H::g2_inf(), Q[1]}, "identities only", 1)) return 1;
    }
    if (argc > 2) {   // the EIP-197 known answer
        uint64_t w[48];
        const char* s = argv[2];
        for (int i = 0; i < 48; ++i) {
            char* end = nullptr;
            w[i] = strtoull(s, &end, 16);
            CHECK(end != s, "argv[2] holds %d words", i);
            s = end;
        }
        const H::G1 p1 = H::g1_from_wire(w), p2 = H::g1_from_wire(w + 24);
        const H::G2 q1 = H::g2_from_wire(w + 8), q2 = H::g2_from_wire(w + 32);
        CHECK(H::g1_on_curve(p1) && H::g1_on_curve(p2) && H::g2_on_curve(q1) && H::g2_on_curve(q2), "known answer: a point is off its curve");
        if (check_vs_host({p1, p2}, {q1, q2}, "EIP-197 vector", 1)) return 1;
        if (check_vs_host({p1, H::g1_neg(p2)}, {q1, q2}, "EIP-197 vector, second point negated", 0)) return 1;
        if (check_vs_host({p1, p2}, {q2, q1}, "EIP-197 vector, G2 points swapped", 0)) return 1;
    }
    {   // points off their curves are flagged, G1 as 1 and G2 as 2
        uint64_t a[8], b[16];
        H::g1_to_wire(P[0], a); H::g2_to_wire(Q[0], b);
        uint32_t aw[16], bw[32], o1[16], o2[32];
        memcpy(aw, a, 64); memcpy(bw, b, 128);
        CHECK(pairing_pair_to_device(o1, o2, aw, bw) == 0, "a good pair is flagged");
        aw[0] ^= 1;
        CHECK(pairing_pair_to_device(o1, o2, aw, bw) == 1, "G1 off the curve");
        bw[17] ^= 4;
        CHECK(pairing_pair_to_device(o1, o2, aw, bw) == 3, "both off their curves");
        aw[0] ^= 1;
        CHECK(pairing_pair_to_device(o1, o2, aw, bw) == 2, "G2 off the twist");
        memset(aw, 0, 64); memset(bw, 0, 128);
        CHECK(pairing_pair_to_device(o1, o2, aw, bw) == 0, "identities are flagged");
    }
    {   // the argument table of the batched entries, in its order
        int dummy = 0;
        uint64_t off[4] = {0, 2, 2, 5}, pts[1] = {0};
        size_t total = 77;
        uint8_t out[4];
        CHECK(H::pairing_batch_check_args(nullptr, pts, pts, off, 3, out, &total) == KZG_ERR_INVALID_ARG && total == 0, "null context");
        CHECK(H::pairing_batch_check_args(&dummy, pts, pts, nullptr, 3, out, &total) == KZG_ERR_INVALID_ARG, "null offsets");
        CHECK(H::pairing_batch_check_args(&dummy, pts, pts, off, 3, nullptr, &total) == KZG_ERR_INVALID_ARG, "null output");
        CHECK(H::pairing_batch_check_args(&dummy, pts, pts, off, 3, out, &total) == KZG_OK && total == 5, "good arguments");
        CHECK(H::pairing_batch_check_args(&dummy, nullptr, pts, off, 3, out, &total) == KZG_ERR_INVALID_ARG, "null G1 array");
        CHECK(H::pairing_batch_check_args(&dummy, pts, nullptr, off, 3, out, &total) == KZG_ERR_INVALID_ARG, "null G2 array");
        CHECK(H::pairing_batch_check_args(&dummy, nullptr, nullptr, off, 0, nullptr, &total) == KZG_OK && total == 0, "no checks");
        uint64_t empty[3] = {0, 0, 0};
        CHECK(H::pairing_batch_check_args(&dummy, nullptr, nullptr, empty, 2, out, &total) == KZG_OK && total == 0, "empty checks need no points");
        uint64_t late[3] = {1, 2, 3}, down[4] = {0, 3, 2, 5};
        CHECK(H::pairing_batch_check_args(&dummy, pts, pts, late, 2, out, &total) == KZG_ERR_INVALID_ARG, "offsets start at 1");
        CHECK(H::pairing_batch_check_args(&dummy, pts, pts, down, 3, out, &total) == KZG_ERR_INVALID_ARG, "offsets decrease");
        uint64_t longc[2] = {0, H::PAIRING_BATCH_MAX_PAIRS_PER_CHECK + 1};
        CHECK(H::pairing_batch_check_args(&dummy, pts, pts, longc, 1, out, &total) == KZG_ERR_TOO_LARGE, "a check too long");
        longc[1] = H::PAIRING_BATCH_MAX_PAIRS_PER_CHECK;
        CHECK(H::pairing_batch_check_args(&dummy, pts, pts, longc, 1, out, &total) == KZG_OK, "a check at the limit");
        CHECK(H::pairing_batch_check_args(&dummy, pts, pts, off, H::PAIRING_BATCH_MAX_CHECKS + 1, out, &total) == KZG_ERR_TOO_LARGE, "too many checks");
        std::vector<uint64_t> many(H::PAIRING_BATCH_MAX_PAIRS / 64 + 2);
        for (size_t i = 0; i < many.size(); ++i) many[i] = 64 * i;
        CHECK(H::pairing_batch_check_args(&dummy, pts, pts, many.data(), many.size() - 1, out, &total) == KZG_ERR_TOO_LARGE, "too many pairs");
        CHECK(H::pairing_batch_check_args(&dummy, pts, pts, many.data(), many.size() - 2, out, &total) == KZG_OK && total == H::PAIRING_BATCH_MAX_PAIRS, "pairs at the limit");
        for (size_t n : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)4096}) {
            const H::PairingBatchPlan p = H::pairing_batch_plan(n, 2 * n + 1);
            CHECK(p.check_blocks * (size_t)H::PAIRING_BLOCK >= n && (n == 0 || (p.check_blocks - 1) * (size_t)H::PAIRING_BLOCK < n), "check blocks of %zu", n);
            CHECK(p.wire_g2 >= 64 * p.total && p.wire_bytes >= p.wire_g2 + 128 * p.total, "wire layout of %zu", n);
            CHECK(p.dev_g2 >= 64 * p.total && p.dev_offsets >= p.dev_g2 + 128 * p.total && p.dev_flags >= p.dev_offsets + 4 * (n + 1) && p.dev_bytes >= p.dev_flags + p.total, "device layout of %zu", n);
            CHECK(p.out_ok >= 384 * n && p.out_bytes >= p.out_ok + n, "output layout of %zu", n);
        }
    }
    printf("pairingdevcheck ok\n");
    return 0;
}
