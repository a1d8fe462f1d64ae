// tests/hostcheck/g1decodecheck.cpp — TEST-ONLY stand-alone program: the strict device decoder of gnark-compressed G1 points
// (csrc/g1_decode.h: flags, canonical x, the square root by the 3-bit window of g2_decode.h, the sign rule), the scalar decoder beside it
// and the second producer of csrc/coset_item_stream.h, compiled by g++ with -DKZG_BOUND_CHECK (every lazy-reduction bound aborts).
// Run by tests/test_coset_bytes_host.py, once as it is and once under -fsanitize=address,undefined.
//
// argv[1] = a file of records written by the test with big integers: 32 input bytes, 1 byte expected kind (0 deserialize, 1 not on
// curve, 4 a finite point, 5 the identity), 64 bytes expected x || y big-endian canonical (zeros unless kind 4).  Every record must
// decode to its kind and coordinates; every finite point must encode back to its bytes with the host encoder (csrc/host_coset_bytes.h).
// Prints "g1 decode ok records=<n> finite=<n> identity=<n> deserialize=<n> not_on_curve=<n>" and exits 0 when every answer is the expected one.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "g1_decode.h"
#include "coset_item_stream.h"
#include "host_g2_decode.h"
#include "host_coset_bytes.h"

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

static void be32_of_plain(uint8_t out[32], const uint64_t w[4]) { for (int i = 0; i < 4; ++i) H::put_u64be(out + 8 * i, w[3 - i]); }
static void fq_be(uint8_t out[32], const Fq& a) {                      // internal form, canonical -> big-endian bytes of the integer
    uint32_t w[8];
    fe_to_wire(w, a);
    H::Fq m;
    memcpy(m.l, w, 32);
    const H::Fq p = H::fq_to_plain(m);
    be32_of_plain(out, p.l);
}

// ---- scalars ---------------------------------------------------------------------------------------------------------------------
static void check_scalar(const uint64_t plain[4], bool want_below) {
    uint8_t b[32];
    be32_of_plain(b, plain);
    uint32_t raw[8], out[8];
    g1_bytes_to_words(raw, b);
    const bool below = fr_decode_be_to_wire(out, raw);
    EXPECT(below == want_below, "fr_decode_be_to_wire: below = %d, expected %d", (int)below, (int)want_below);
    if (!want_below) return;
    uint64_t want[4], got[4];
    H::fr_mul(plain, H::FR_R2, want);                                   // canonical -> Montgomery
    memcpy(got, out, 32);
    EXPECT(memcmp(got, want, 32) == 0, "fr_decode_be_to_wire: not the Montgomery form of the integer");
    uint8_t back[32];
    EXPECT(H::fr_encode_be(got, back) && memcmp(back, b, 32) == 0, "fr_encode_be does not give the bytes back");
}

// ---- the second producer of the item message ---------------------------------------------------------------------------------------
static void check_item_stream(const std::vector<uint8_t>& proofs, size_t n_proofs) {
    const uint32_t ls[4] = {1, 2, 16, 64};
    for (uint32_t l : ls)
        for (size_t it = 0; it < 6 && it < n_proofs; ++it) {
            alignas(16) uint8_t ys[64 * 32];
            for (size_t k = 0; k < 32 * (size_t)l; ++k) ys[k] = (uint8_t)next64();
            alignas(16) uint8_t proof[32];
            memcpy(proof, proofs.data() + 32 * ((it * 7) % n_proofs), 32);
            if (it == 5) { memset(proof, 0, 32); proof[0] = 0x40; }    // the identity
            const uint64_t c = next64() >> 40, k = next64() >> 44;
            // the host's message, byte by byte
            std::vector<uint8_t> msg(72 + 32 * (size_t)l);
            memcpy(msg.data(), H::COSET_ITEM_DOMAIN, 24);
            H::put_u64be(msg.data() + 24, c);
            H::put_u64be(msg.data() + 32, k);
            memcpy(msg.data() + 40, ys, 32 * (size_t)l);
            H::gnark_to_ark(proof, msg.data() + 40 + 32 * (size_t)l);
            const size_t total = msg.size();
            const uint32_t nb = coset_item_blocks(l);
            std::vector<uint8_t> padded((size_t)nb * 64, 0);
            memcpy(padded.data(), msg.data(), total);
            padded[total] = 0x80;
            H::put_u64be(padded.data() + padded.size() - 8, (uint64_t)total * 8);
            CosetItemBytesSrc src;
            src.ys = reinterpret_cast<const uint32_t*>(ys);
            src.proof = reinterpret_cast<const uint32_t*>(proof);
            src.c = c; src.k = k; src.l = l;
            uint32_t carry[2] = {0, 0}, w[16];
            for (uint32_t b = 0; b < nb; ++b) {
                coset_item_bytes_block(w, src, b, carry);
                for (int j = 0; j < 16; ++j) {
                    const uint8_t* q = padded.data() + 64 * (size_t)b + 4 * j;
                    const uint32_t want = (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | q[3];
                    EXPECT(w[j] == want, "item stream from bytes: l = %u, block %u, word %d", l, b, j);
                }
            }
        }
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: g1decodecheck <file of records>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> data;
    uint8_t buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) != 0;) data.insert(data.end(), buf, buf + k);
    fclose(f);
    const size_t REC = 32 + 1 + 64;
    if (data.empty() || data.size() % REC != 0) { fprintf(stderr, "not a multiple of %zu bytes\n", REC); return 1; }
    const size_t n = data.size() / REC;
    size_t counts[6] = {0, 0, 0, 0, 0, 0};
    std::vector<uint8_t> finite;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* rec = data.data() + REC * i;
        const uint32_t want = rec[32];
        uint32_t raw[8];
        g1_bytes_to_words(raw, rec);
        Fq x, y;
        const uint32_t kind = g1_decompress_point(x, y, raw);
        EXPECT(kind == want, "record %zu: kind %u, expected %u", i, kind, want);
        if (kind < 6) ++counts[kind];
        if (kind == G1_DECODE_IDENTITY) {
            uint32_t o[16];
            g1_point_to_device_words(o, x, y);
            uint32_t any = 0;
            for (int j = 0; j < 16; ++j) any |= o[j];
            EXPECT(any == 0, "record %zu: the identity is not 16 zero words", i);
        }
        if (kind != G1_DECODE_OK || want != G1_DECODE_OK) continue;
        EXPECT(fe_bound_pack(x) && fe_bound_pack(y), "record %zu: coordinates not canonical", i);
        uint8_t xb[32], yb[32];
        fq_be(xb, x);
        fq_be(yb, y);
        EXPECT(memcmp(xb, rec + 33, 32) == 0, "record %zu: x differs", i);
        EXPECT(memcmp(yb, rec + 65, 32) == 0, "record %zu: y differs", i);
        uint32_t wire[16];
        g1_point_to_wire_words(wire, x, y);
        uint64_t xy[8];
        memcpy(xy, wire, 64);
        EXPECT(H::g1_on_curve(H::g1_from_wire(xy)), "record %zu: the wire point is not on the curve", i);
        uint8_t back[32];
        EXPECT(H::g1_encode_be(xy, back) && memcmp(back, rec, 32) == 0, "record %zu: the host encoder does not give the bytes back", i);
        // the ark form from the bytes equals the ark form from the point (what makes the two transcripts one)
        uint8_t ark_bytes[32], ark_point[32];
        H::gnark_to_ark(rec, ark_bytes);
        H::g1_serialize_compressed_ark(H::g1_from_wire(xy), ark_point);
        EXPECT(memcmp(ark_bytes, ark_point, 32) == 0, "record %zu: gnark_to_ark differs from the serialised point", i);
        if (finite.size() < 64 * 32) finite.insert(finite.end(), rec, rec + 32);
    }
    {   // the identity through the host encoder and the ark map
        const uint64_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint8_t b[32], ark_bytes[32], ark_point[32];
        EXPECT(H::g1_encode_be(zero, b) && b[0] == 0x40, "the all-zero wire point does not encode as 0x40 || zeros");
        for (int k = 1; k < 32; ++k) EXPECT(b[k] == 0, "the all-zero wire point does not encode as 0x40 || zeros");
        H::gnark_to_ark(b, ark_bytes);
        H::g1_serialize_compressed_ark(H::g1_from_wire(zero), ark_point);
        EXPECT(memcmp(ark_bytes, ark_point, 32) == 0, "gnark_to_ark of the identity");
        uint64_t big[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        memcpy(big, H::FQ_P.l, 32);                                     // x = p as wire words: not below the modulus
        big[4] = 1;
        EXPECT(!H::g1_encode_be(big, b), "a coordinate equal to p was encoded");
    }
    // scalars: 0, 1, r - 1, r, r + 1, 2^256 - 1, random
    {
        uint64_t r[4], t[4];
        memcpy(r, H::FR_MODULUS_WORDS, 32);
        const uint64_t zero[4] = {0, 0, 0, 0}, one[4] = {1, 0, 0, 0}, ones[4] = {~0ULL, ~0ULL, ~0ULL, ~0ULL};
        check_scalar(zero, true);
        check_scalar(one, true);
        memcpy(t, r, 32); t[0] -= 1; check_scalar(t, true);
        check_scalar(r, false);
        memcpy(t, r, 32); t[0] += 1; check_scalar(t, false);
        check_scalar(ones, false);
        memcpy(t, r, 32); t[3] += 1; check_scalar(t, false);           // above r in the top word only
        memcpy(t, r, 32); t[3] -= 1; t[0] = ~0ULL; check_scalar(t, true);   // below r in the top word only
        for (int k = 0; k < 300; ++k) {
            uint64_t v[4] = {next64(), next64(), next64(), next64() >> 2};
            check_scalar(v, !H::fr_geq_r(v));
        }
        EXPECT(!H::fr_encode_be(r, buf), "a value equal to r was encoded");
    }
    if (!finite.empty()) check_item_stream(finite, finite.size() / 32);
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    printf("g1 decode ok records=%zu finite=%zu identity=%zu deserialize=%zu not_on_curve=%zu\n", n, counts[G1_DECODE_OK], counts[G1_DECODE_IDENTITY],
           counts[G1_BAD_DESERIALIZE], counts[G1_BAD_NOT_ON_CURVE]);
    return 0;
}
