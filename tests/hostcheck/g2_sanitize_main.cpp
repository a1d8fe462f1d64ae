// tests/hostcheck/g2_sanitize_main.cpp — TEST-ONLY stand-alone program for g++ -fsanitize=address,undefined: the host code of the G2
// feature that reads caller bytes or sizes plans -- the decoder of gnark-compressed G2 points (csrc/host_g2_decode.h) over a file given
// on the command line and over damaged copies of its first points, and the G2 MSM planner over the grid of g2msm_plan_grid.h.  Prints
// "g2 sanitize ok <points>" and exits 0 when every answer is the expected one.  Run by tests/test_g2_decode_host.py as a subprocess;
// nothing is loaded into Python.
#include <cstdio>
#include <cstring>
#include <vector>

#include "g2msm_plan_grid.h"
#include "host_g2_decode.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: g2_sanitize_main <file of 64-byte compressed G2 points>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> data;
    uint8_t buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) != 0;) data.insert(data.end(), buf, buf + k);
    fclose(f);
    if (data.empty() || data.size() % 64 != 0) { fprintf(stderr, "not a multiple of 64 bytes\n"); return 1; }
    const size_t n = data.size() / 64;
    int bad = 0;
    for (size_t i = 0; i < n; ++i) {
        kzg_host::G2 p;
        if (kzg_host::g2_decompress_be(data.data() + 64 * i, p) != KZG_OK || !kzg_host::g2_on_curve(p)) { fprintf(stderr, "point %zu does not decode\n", i); ++bad; }
    }
    // damaged copies of the first point: flag bits, a coordinate at the modulus, the other y, an x without a point
    {
        uint8_t c[64];
        kzg_host::G2 p, q;
        memcpy(c, data.data(), 64); c[0] &= 0x3F;
        if (kzg_host::g2_decompress_be(c, p) != KZG_ERR_DESERIALIZE) { fprintf(stderr, "flag 0 accepted\n"); ++bad; }
        memcpy(c, data.data(), 64); c[0] = (uint8_t)((c[0] & 0x3F) | 0x40);
        if (kzg_host::g2_decompress_be(c, p) != KZG_ERR_DESERIALIZE) { fprintf(stderr, "flag 1 accepted\n"); ++bad; }
        memcpy(c, data.data(), 64); memset(c + 32, 0xFF, 32);
        if (kzg_host::g2_decompress_be(c, p) != KZG_ERR_DESERIALIZE) { fprintf(stderr, "x.c0 >= p accepted\n"); ++bad; }
        memcpy(c, data.data(), 64); c[0] ^= 0x40;                        // 0b10 <-> 0b11: the negated point
        if (kzg_host::g2_decompress_be(data.data(), p) != KZG_OK || kzg_host::g2_decompress_be(c, q) != KZG_OK || !kzg_host::g2_add(p, q).inf) { fprintf(stderr, "the other flag is not the negated point\n"); ++bad; }
        int off = 0;
        for (int t = 1; t < 40 && !off; ++t) {                            // about half of all x have no point on the twist
            memcpy(c, data.data(), 64); c[63] = (uint8_t)(c[63] + t);
            if (kzg_host::g2_decompress_be(c, p) == KZG_ERR_NOT_ON_CURVE) off = 1;
        }
        if (!off) { fprintf(stderr, "no x without a point among 39 neighbours\n"); ++bad; }
    }
    bad += g2grid::run(nullptr);
    if (bad) return 1;
    printf("g2 sanitize ok %zu\n", n);
    return 0;
}
