// host_header_bytes.h — blob headers in their SERIALIZED form, the host side: the encoder (the disperser's half, kzg_header_items_encode_be).
// Wire format: the commitment is a 32-byte gnark-compressed G1 point (host_coset_bytes.h g1_encode_be), the length
// commitment and the length proof are 64-byte gnark-compressed G2 points, X.A1 || X.A0 big-endian, the top two bits of byte 0: 0b10 / 0b11
// the smaller / larger y by LexicographicallyLargest on (y.c1, y.c0) (host_g2_decode.h), 0b01 the identity, written 0x40 || 63 zero bytes.
// Pure host code (no HIP, no engine.h); also compiled with g++ under sanitizers by tests/hostcheck/header_bytes_sanitize_main.cpp.
#pragma once
#include "host_coset_bytes.h"
#include "host_g2_decode.h"

namespace kzg_host {

// one wire point -> 64 gnark-compressed bytes; the all-zero wire point -> 0x40 || zeros; false: a coordinate is not below p
inline bool g2_encode_be(const uint64_t wire[16], uint8_t out[64]) {
    const G2 p = g2_from_wire(wire);
    memset(out, 0, 64);
    if (p.inf) { out[0] = 0x40; return true; }
    if (geq_p(p.x.c0) || geq_p(p.x.c1) || geq_p(p.y.c0) || geq_p(p.y.c1)) return false;
    const Fq a1 = fq_to_plain(p.x.c1), a0 = fq_to_plain(p.x.c0);
    for (int i = 0; i < 4; ++i) { put_u64be(out + 8 * i, a1.l[3 - i]); put_u64be(out + 32 + 8 * i, a0.l[3 - i]); }
    out[0] |= fq2_lexicographically_largest(p.y) ? 0xC0 : 0x80;                          // x.c1 < p < 2^254 leaves the two top bits free
    return true;
}

}  // namespace kzg_host
