// tests/hostcheck/g1compresscheck.cpp — TEST-ONLY stand-alone program: the device compressor of G1 points (csrc/g1_decode.h
// g1_compress_point, g1_compress_wire_point), the way out that the encoder's byte stores take, compiled by g++ with -DKZG_BOUND_CHECK
// (every lazy-reduction bound aborts).  Run by tests/test_encode_bytes_host.py, once as it is and once under -fsanitize=address,undefined.
//
// argv[1] = a file of records written by the test with big integers: 64 bytes x || y big-endian canonical (all zeros: the identity),
// then the 32 bytes the point compresses to.  For every record: g1_compress_wire_point of the wire point gives those bytes, so does the
// host encoder (csrc/host_coset_bytes.h g1_encode_be); g1_decompress_point of the bytes gives the point back, and compressing THAT
// (the internal form, what the affine conversion holds) gives the bytes again.  For a finite point the negative differs in the flag alone.
// Prints "g1 compress ok records=<n> identity=<n> small=<n> large=<n>" and exits 0 when every answer is the expected one.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "g1_decode.h"
#include "host_g2_decode.h"
#include "host_coset_bytes.h"

using namespace kzg;
namespace H = kzg_host;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (++failures <= 20) { fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static H::Fq plain_of_be(const uint8_t b[32]) {
    H::Fq v;
    for (int i = 0; i < 4; ++i) {
        uint64_t w = 0;
        for (int j = 0; j < 8; ++j) w = w << 8 | b[8 * i + j];
        v.l[3 - i] = w;
    }
    return v;
}
static void words_to_bytes(uint8_t out[32], const uint32_t raw[8]) {       // the little-endian store the kernels do
    for (int j = 0; j < 8; ++j)
        for (int k = 0; k < 4; ++k) out[4 * j + k] = (uint8_t)(raw[j] >> (8 * k));
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: g1compresscheck <file of records>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> data;
    uint8_t buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) != 0;) data.insert(data.end(), buf, buf + k);
    fclose(f);
    const size_t REC = 64 + 32;
    if (data.empty() || data.size() % REC != 0) { fprintf(stderr, "not a multiple of %zu bytes\n", REC); return 1; }
    const size_t n = data.size() / REC;
    size_t identity = 0, small = 0, large = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* rec = data.data() + REC * i;
        const uint8_t* want = rec + 64;
        bool is_identity = true;
        for (int k = 0; k < 64; ++k) is_identity = is_identity && rec[k] == 0;
        uint64_t xy[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (!is_identity) {
            const H::Fq x = H::fq_from_plain(plain_of_be(rec)), y = H::fq_from_plain(plain_of_be(rec + 32));
            memcpy(xy, x.l, 32);
            memcpy(xy + 4, y.l, 32);
        }
        // the host encoder
        uint8_t host[32];
        EXPECT(H::g1_encode_be(xy, host) && memcmp(host, want, 32) == 0, "record %zu: the host encoder differs from the big integers", i);
        // the device compressor from the wire point
        uint32_t wire[16], raw[8];
        memcpy(wire, xy, 64);
        g1_compress_wire_point(raw, wire);
        uint8_t got[32];
        words_to_bytes(got, raw);
        EXPECT(memcmp(got, want, 32) == 0, "record %zu: g1_compress_wire_point differs", i);
        // the round trip: decompress, and compress the internal form the decoder leaves
        uint32_t in[8];
        g1_bytes_to_words(in, want);
        Fq x, y;
        const uint32_t kind = g1_decompress_point(x, y, in);
        EXPECT(kind == (is_identity ? G1_DECODE_IDENTITY : G1_DECODE_OK), "record %zu: the bytes decode to kind %u", i, kind);
        uint32_t back_wire[16];
        g1_point_to_wire_words(back_wire, x, y);
        EXPECT(memcmp(back_wire, wire, 64) == 0, "record %zu: g1_decompress_point(g1_compress_point(P)) != P", i);
        uint32_t raw2[8];
        g1_compress_point(raw2, x, y, kind == G1_DECODE_IDENTITY);
        EXPECT(memcmp(raw2, raw, 32) == 0, "record %zu: compressing the decoded point differs", i);
        if (is_identity) {
            ++identity;
            EXPECT(want[0] == 0x40, "record %zu: the identity is not 0x40 || zeros", i);
            continue;
        }
        (want[0] >> 6) == 3 ? ++large : ++small;
        // the negative: the same x, the other flag
        Fq ny;
        fe_cneg(ny, y, 1u);                        // y canonical: -y in (-m, 0]
        fe_norm(ny);
        uint32_t rawn[8];
        g1_compress_point(rawn, x, ny, false);
        EXPECT((rawn[0] ^ raw[0]) == 0x40u, "record %zu: a point and its negative do not differ in the flag alone", i);
        for (int k = 1; k < 8; ++k) EXPECT(rawn[k] == raw[k], "record %zu: a point and its negative differ in x", i);
    }
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    printf("g1 compress ok records=%zu identity=%zu small=%zu large=%zu\n", n, identity, small, large);
    return 0;
}
