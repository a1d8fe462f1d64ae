// tests/hostcheck/g2sqrtcheck.cpp — TEST-ONLY stand-alone program: the device decoder of gnark-compressed G2 points (csrc/g2_decode.h:
// byte decode, square roots in Fq and Fq2, sign rule, one point) compiled by g++ with -DKZG_BOUND_CHECK (every lazy-reduction bound
// aborts) and compared BY VALUE with the independent Fq / Fq2 of csrc/host_pairing.h and the host decoder of csrc/host_g2_decode.h
// (4 x 64-bit Montgomery limbs, three exponentiations).  Run by tests/test_g2_sqrt_host.py, once as it is and once under
// -fsanitize=address,undefined; argv[1] = a file of 64-byte compressed G2 points.  Prints
// "g2 sqrt ok direct=<n> swapped=<n> none=<n> points=<n>" and exits 0 when every answer is the expected one.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "g2_decode.h"
#include "host_g2_decode.h"

using namespace kzg;
namespace H = kzg_host;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (++failures <= 20) { fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t next64() {                         // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static H::Fq random_fq() {                         // uniform below p (any such words are the Montgomery form of some element)
    for (;;) {
        H::Fq v = {{next64(), next64(), next64(), next64() & 0x3FFFFFFFFFFFFFFFULL}};
        if (!H::geq_p(v)) return v;
    }
}
static Fq dev_of(const H::Fq& a) { Fq r; fe_from_wire(r, reinterpret_cast<const uint32_t*>(a.l)); return r; }                  // class F
static Fq2 dev_of(const H::Fq2& a) { Fq2 r; r.c0 = dev_of(a.c0); r.c1 = dev_of(a.c1); return r; }
static H::Fq host_of(const Fq& a) { uint32_t w[8]; fe_to_wire(w, a); H::Fq r; memcpy(r.l, w, 32); return r; }
static H::Fq2 host_of(const Fq2& a) { return {host_of(a.c0), host_of(a.c1)}; }
static bool class_f(const Fq& a) { return fe_bound_canon(a); }
static H::Fq host_half(const H::Fq& a) { H::Fq s = a; H::half_mod_p(s); return s; }

// ---- Fq ------------------------------------------------------------------------------------------------------------------------
static void check_fq_sqrt(const H::Fq& a) {
    Fq r;
    const bool got = fq_sqrt_candidate(r, dev_of(a));
    H::Fq want;
    const bool has = H::fq_sqrt(a, want);
    EXPECT(class_f(r), "fq_sqrt_candidate leaves class F");
    EXPECT(got == has, "fq_sqrt_candidate: residue answer %d, host %d", (int)got, (int)has);
    const H::Fq hr = host_of(r);
    EXPECT(H::eq(hr, want), "fq_sqrt_candidate: not the host's a^((p+1)/4)");
    EXPECT(H::eq(H::sqr(hr), has ? a : H::neg(a)), "fq_sqrt_candidate: r^2 is neither a nor -a");
}

// ---- Fq2 -----------------------------------------------------------------------------------------------------------------------
static int n_direct = 0, n_swapped = 0, n_none = 0;
// the branch a takes by the host's arithmetic: 0 direct, 1 swapped, 2 not a square (a1 != 0)
static int host_branch(const H::Fq2& a, H::Fq& delta) {
    H::Fq alpha, x0;
    if (!H::fq_sqrt(H::add(H::sqr(a.c0), H::sqr(a.c1)), alpha)) return 2;
    delta = host_half(H::add(a.c0, alpha));
    return H::fq_sqrt(delta, x0) ? 0 : 1;
}
static void check_fq2_sqrt(const H::Fq2& a, bool count) {
    Fq2 r;
    const bool got = fq2_sqrt(r, dev_of(a));
    H::Fq2 want;
    const bool has = H::fq2_sqrt(a, want);
    EXPECT(got == has, "fq2_sqrt: square answer %d, host %d", (int)got, (int)has);
    EXPECT(class_f(r.c0) && class_f(r.c1), "fq2_sqrt leaves class F");
    if (!got) { if (count) ++n_none; return; }
    const H::Fq2 hr = host_of(r);
    EXPECT(H::eq(H::sqr(hr), a), "fq2_sqrt: the root does not square to its input");
    EXPECT(H::eq(hr, want) || H::eq(hr, H::neg(want)), "fq2_sqrt: not +- the host's root");
    if (H::is_zero(a.c1)) {
        H::Fq t;
        if (H::fq_sqrt(a.c0, t)) EXPECT(H::is_zero(hr.c1), "a1 = 0, a0 a residue: the root is (sqrt(a0), 0)");
        else EXPECT(H::is_zero(hr.c0), "a1 = 0, a0 not a residue: the root is (0, sqrt(-a0))");
        return;
    }
    H::Fq delta;
    const int br = host_branch(a, delta);
    EXPECT(br != 2, "a square with a norm that is none");
    if (br == 0) EXPECT(H::eq(H::sqr(hr.c0), delta), "direct branch: c0^2 == delta");
    else EXPECT(H::eq(H::sqr(hr.c1), H::neg(delta)), "swapped branch: c1^2 == -delta");
    if (count) { if (br == 0) ++n_direct; else ++n_swapped; }
}

// ---- sign rule -------------------------------------------------------------------------------------------------------------------
static void check_sign_rule() {
    H::Fq half = H::FQ_P; H::shr1(half);                                    // (p - 1) / 2
    H::Fq half_up = half; half_up.l[0] += 1;                                // (p + 1) / 2 (no carry: the low word of (p - 1) / 2 is ..a3)
    H::Fq pm1 = H::FQ_P; pm1.l[0] -= 1;
    const H::Fq plain[6] = {{{0, 0, 0, 0}}, {{1, 0, 0, 0}}, half, half_up, pm1, {{2, 0, 0, 0}}};
    const bool large[6] = {false, false, false, true, true, false};
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            const H::Fq2 y = {H::fq_from_plain(plain[i]), H::fq_from_plain(plain[j])};
            const bool got = fq2_lexicographically_largest(dev_of(y));
            EXPECT(got == H::fq2_lexicographically_largest(y), "sign rule differs from the host's at c0 #%d, c1 #%d", i, j);
            EXPECT(got == (j == 0 ? large[i] : large[j]), "sign rule: c0 #%d, c1 #%d", i, j);
        }
    for (int k = 0; k < 200; ++k) {
        const H::Fq2 y = {random_fq(), k % 5 == 0 ? H::fq_zero() : random_fq()};
        EXPECT(fq2_lexicographically_largest(dev_of(y)) == H::fq2_lexicographically_largest(y), "sign rule differs from the host's on a random y");
    }
}

// ---- bytes and whole points ---------------------------------------------------------------------------------------------------
static void be32(uint8_t out[32], const H::Fq& a) {
    const H::Fq p = H::fq_to_plain(a);
    for (int j = 0; j < 4; ++j) for (int k = 0; k < 8; ++k) out[8 * (3 - j) + k] = (uint8_t)(p.l[j] >> (8 * (7 - k)));
}
static void compress(uint8_t out[64], const H::Fq2& x, int flag) { be32(out, x.c1); be32(out + 32, x.c0); out[0] = (uint8_t)(out[0] | flag << 6); }
static uint32_t decode(G2Affine& p, const uint8_t ch[64]) { uint32_t raw[16]; g2_bytes_to_words(raw, ch); return g2_decompress_point(p, raw); }
// the device decoder's answer for the bytes against the host's arithmetic; returns the kind
static uint32_t check_point(const uint8_t ch[64]) {
    G2Affine p;
    const uint32_t kind = decode(p, ch);
    const int flag = ch[0] >> 6;
    H::Fq2 x;
    const bool wellformed = (flag == 2 || flag == 3) && H::fq_from_be(ch + 32, 0xFF, x.c0) && H::fq_from_be(ch, 0x3F, x.c1);
    EXPECT((kind == G2_BAD_DESERIALIZE) == !wellformed, "deserialisation answer differs from the host's");
    if (!wellformed || kind == G2_BAD_DESERIALIZE) return kind;
    H::Fq2 y;
    const H::Fq2 b = {H::TWIST_B0, H::TWIST_B1};
    const bool has = H::fq2_sqrt(H::add(H::mul(H::sqr(x), x), b), y);
    EXPECT((kind == G2_DECODE_OK) == has, "a point of that x exists: device %d, host %d", (int)(kind == G2_DECODE_OK), (int)has);
    if (kind != G2_DECODE_OK || !has) { EXPECT(kind == G2_DECODE_OK || kind == G2_BAD_NO_POINT, "kind %u", kind); return kind; }
    if ((flag == 3) != H::fq2_lexicographically_largest(y)) y = H::neg(y);
    EXPECT(fe_bound_pack(p.x.c0) && fe_bound_pack(p.x.c1) && fe_bound_pack(p.y.c0) && fe_bound_pack(p.y.c1), "coordinates not canonical");
    EXPECT(H::eq(host_of(p.x), x), "x differs from the host's");
    EXPECT(H::eq(host_of(p.y), y), "y differs from the host's");
    EXPECT(g2_on_twist(p.x, p.y), "not on the twist");
    return kind;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: g2sqrtcheck <file of 64-byte compressed G2 points>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> data;
    uint8_t buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) != 0;) data.insert(data.end(), buf, buf + k);
    fclose(f);
    if (data.empty() || data.size() % 64 != 0) { fprintf(stderr, "not a multiple of 64 bytes\n"); return 1; }
    const size_t n = data.size() / 64;

    // Fq: 0, 1, -1, residues and non-residues
    check_fq_sqrt(H::fq_zero());
    check_fq_sqrt(H::FQ_ONE);
    check_fq_sqrt(H::neg(H::FQ_ONE));
    for (int k = 0; k < 300; ++k) check_fq_sqrt(random_fq());
    { Fq h, two; fq_set_half(h); fe_set_one(two); fe_dbl(two, two); fe_norm(two); Fq pr; fe_mul(pr, h, two); EXPECT(H::eq(host_of(pr), H::FQ_ONE), "fq_set_half is not 1 / 2"); }

    // Fq2: 0, 1, -1 = u^2, a1 = 0 with a0 a residue / not a residue, random elements, squares of random elements
    const H::Fq z = H::fq_zero();
    check_fq2_sqrt({z, z}, false);
    check_fq2_sqrt({H::FQ_ONE, z}, false);
    check_fq2_sqrt({H::neg(H::FQ_ONE), z}, false);
    { Fq2 r; EXPECT(fq2_sqrt(r, dev_of(H::Fq2{H::neg(H::FQ_ONE), z})) && H::is_zero(host_of(r.c0)) && H::eq(H::sqr(host_of(r.c1)), H::FQ_ONE), "sqrt(-1) is +-u"); }
    { Fq2 r; EXPECT(fq2_sqrt(r, dev_of(H::Fq2{z, z})) && H::is_zero(host_of(r.c0)) && H::is_zero(host_of(r.c1)), "sqrt(0) is 0"); }
    for (int k = 0; k < 40; ++k) {
        const H::Fq t2 = H::sqr(random_fq());
        check_fq2_sqrt({t2, z}, false);                                     // a0 a residue
        check_fq2_sqrt({H::neg(t2), z}, false);                             // a0 not a residue (-1 is none)
        check_fq2_sqrt({z, t2}, false);                                     // a0 = 0
    }
    for (int k = 0; k < 2400; ++k) check_fq2_sqrt({random_fq(), random_fq()}, true);
    for (int k = 0; k < 300; ++k) {
        const H::Fq2 t = {random_fq(), k % 7 == 0 ? z : random_fq()};
        Fq2 r;
        const bool got = fq2_sqrt(r, dev_of(H::sqr(t)));
        const H::Fq2 hr = host_of(r);
        EXPECT(got && (H::eq(hr, t) || H::eq(hr, H::neg(t))), "the root of t^2 is not +-t");
        check_fq2_sqrt(H::sqr(t), false);
    }
    EXPECT(n_direct >= 100 && n_swapped >= 100 && n_none >= 100 && n_direct + n_swapped + n_none >= 2000, "branch counts %d / %d / %d", n_direct, n_swapped, n_none);

    check_sign_rule();

    // bytes: the points of the file, both flags, against the host decoder; all of them in the subgroup, none the generator
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* ch = data.data() + 64 * i;
        EXPECT(check_point(ch) == G2_DECODE_OK, "point %zu of the file does not decode", i);
        G2Affine p;
        H::G2 hp;
        EXPECT(decode(p, ch) == G2_DECODE_OK && H::g2_decompress_be(ch, hp) == KZG_OK && H::eq(host_of(p.x), hp.x) && H::eq(host_of(p.y), hp.y), "point %zu differs from g2_decompress_be", i);
        if (i < 4) EXPECT(g2_in_subgroup(p) && !g2_is_generator(p), "point %zu: subgroup / generator", i);
        uint8_t c[64];
        memcpy(c, ch, 64); c[0] ^= 0x40;                                    // the other y
        G2Affine q;
        EXPECT(check_point(c) == G2_DECODE_OK && decode(q, c) == G2_DECODE_OK && H::eq(host_of(q.x), hp.x) && H::eq(host_of(q.y), H::neg(hp.y)), "point %zu: the other flag is not the negated point", i);
        { uint32_t raw[16]; Fq2 x; bool below; g2_bytes_to_words(raw, ch); EXPECT(g2_decode_x_be(x, below, raw) == (uint32_t)(ch[0] >> 6) && below, "point %zu: flag bits", i); }
    }
    // the four damage patterns of tests/test_g2_decode_host.py, and an x without a point found by stepping the last byte
    {
        uint8_t c[64];
        memcpy(c, data.data(), 64); c[0] &= 0x3F;
        EXPECT(check_point(c) == G2_BAD_DESERIALIZE, "flag 0b00 accepted");
        memcpy(c, data.data() + 64 * (5 % n), 64); c[0] = (uint8_t)((c[0] & 0x3F) | 0x40);
        EXPECT(check_point(c) == G2_BAD_DESERIALIZE, "flag 0b01 accepted");
        memcpy(c, data.data() + 64 * (n - 1), 64); memset(c + 32, 0xFF, 32);
        EXPECT(check_point(c) == G2_BAD_DESERIALIZE, "x.c0 = 0xff.. accepted");
        memcpy(c, data.data() + 64 * (13 % n), 64); c[0] |= 0x3F; memset(c + 1, 0xFF, 31);
        EXPECT(check_point(c) == G2_BAD_DESERIALIZE, "x.c1 >= p accepted");
        memcpy(c, data.data(), 64); memcpy(c + 32, "\x30\x64\x4e\x72\xe1\x31\xa0\x29\xb8\x50\x45\xb6\x81\x81\x58\x5d\x97\x81\x6a\x91\x68\x71\xca\x8d\x3c\x20\x8c\x16\xd8\x7c\xfd\x47", 32);
        EXPECT(check_point(c) == G2_BAD_DESERIALIZE, "x.c0 = p accepted");
        int off = 0, on = 0;
        for (int t = 1; t < 40; ++t) {
            memcpy(c, data.data() + 64 * (3 % n), 64); c[63] = (uint8_t)(c[63] + t);
            const uint32_t kind = check_point(c);
            off += kind == G2_BAD_NO_POINT; on += kind == G2_DECODE_OK;
        }
        EXPECT(off > 0 && on > 0 && off + on == 39, "stepping the last byte: %d without a point, %d with one", off, on);
    }
    // the generator, compressed here: decodes to itself, and only it is the generator
    {
        const H::G2 g = H::g2_generator();
        uint8_t c[64];
        compress(c, g.x, H::fq2_lexicographically_largest(g.y) ? 3 : 2);
        G2Affine p;
        EXPECT(check_point(c) == G2_DECODE_OK && decode(p, c) == G2_DECODE_OK && H::eq(host_of(p.y), g.y) && g2_is_generator(p) && g2_in_subgroup(p), "the generator");
        c[0] ^= 0x40;
        EXPECT(decode(p, c) == G2_DECODE_OK && !g2_is_generator(p), "the negated generator is not the generator");
    }
    // random x, both flags (points outside the subgroup when they exist); x with x.c1 = 0 and x = 0
    for (int k = 0; k < 120; ++k) {
        const H::Fq2 x = {k == 0 ? z : random_fq(), k % 10 == 0 ? z : random_fq()};
        uint8_t c[64];
        compress(c, x, 2 + (k & 1));
        check_point(c);
    }
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    printf("g2 sqrt ok direct=%d swapped=%d none=%d points=%zu\n", n_direct, n_swapped, n_none, n);
    return 0;
}
