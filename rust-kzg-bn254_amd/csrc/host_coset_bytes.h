// host_coset_bytes.h — coset items in their SERIALIZED form, the host side: the encoder (the disperser's half) and the coset transcript
// read straight from the bytes.  Wire format: a commitment or proof is a 32-byte gnark-compressed G1 point (x
// big-endian, the top two bits of byte 0: 0b01 the identity, 0b10 / 0b11 the smaller / larger y), a value is a 32-byte big-endian
// canonical scalar.  The transcript of host_fiat_shamir.h (multiproof_r_powers_host) hashes be32(value) and the ARK-compressed point;
// for canonical inputs be32(value) is the wire bytes as they are, and the ark form is the gnark bytes reversed with the two flag bits
// remapped (gnark_to_ark below).  So the weights come from the bytes with NO field arithmetic before the final mod r.
// Pure host code (no HIP, no engine.h), like host_fiat_shamir.h.
#pragma once
#include "host_fiat_shamir.h"

namespace kzg_host {

// gnark-compressed -> ark-compressed (x little-endian, flags in the top two bits of the LAST byte: 0x80 = the larger y, 0x40 = the
// identity).  gnark 0b10 -> 0, 0b11 -> 0x80, 0b01 -> 0x40; gnark's 0b00 (no 32-byte point) -> 0xC0, ark's own invalid pair, so that the
// map stays one to one on every byte string: bytes that do not decode are hashed as given.
inline void gnark_to_ark(const uint8_t in[32], uint8_t out[32]) {
    static const uint8_t flag_map[4] = {0xC0, 0x40, 0x00, 0x80};
    for (int k = 0; k < 32; ++k) out[k] = in[31 - k];
    out[31] = (uint8_t)((in[0] & 0x3F) | flag_map[in[0] >> 6]);
}

// coset_batch_transcript (host_fiat_shamir.h) from serialized commitments
inline std::vector<uint8_t> coset_batch_transcript_bytes(const uint8_t* commitments_be, size_t n_commitments, size_t count, size_t n, size_t l) {
    std::vector<uint8_t> data(coset_batch_head(n_commitments) + 32 * count, 0);
    memcpy(data.data(), COSET_BATCH_DOMAIN, 24);
    put_u64be(data.data() + 24, (uint64_t)n);
    put_u64be(data.data() + 32, (uint64_t)l);
    put_u64be(data.data() + 40, (uint64_t)n_commitments);
    put_u64be(data.data() + 48, (uint64_t)count);
    for (size_t c = 0; c < n_commitments; ++c) gnark_to_ark(commitments_be + 32 * c, data.data() + 56 + 32 * c);
    return data;
}
// multiproof_r_powers_host on the encoded form of the same items: equal bits for every input whose bytes decode
inline void multiproof_r_powers_bytes_host(const uint8_t* commitments_be, size_t n_commitments, const uint64_t* commitment_indices, const uint64_t* coset_indices,
                                           const uint8_t* ys_be, const uint8_t* proofs_be, size_t count, size_t n, size_t l, uint64_t* out, ParallelFor parallel_for) {
    const size_t head = coset_batch_head(n_commitments);
    std::vector<uint8_t> data = coset_batch_transcript_bytes(commitments_be, n_commitments, count, n, l);
    const size_t per = std::max<size_t>(1, 1024 / l), jobs = (count + per - 1) / per;
    auto body = [&](size_t j) {
        uint8_t head_bytes[40], tail[32];
        memcpy(head_bytes, COSET_ITEM_DOMAIN, 24);
        for (size_t i = j * per; i < std::min(count, (j + 1) * per); ++i) {
            put_u64be(head_bytes + 24, commitment_indices[i]);
            put_u64be(head_bytes + 32, coset_indices[i]);
            gnark_to_ark(proofs_be + 32 * i, tail);
            Sha256 sh;
            sha256_init(sh);
            sha256_update(sh, head_bytes, 40);
            sha256_update(sh, ys_be + 32 * l * i, 32 * l);                              // the values: the caller's bytes as they are
            sha256_update(sh, tail, 32);
            sha256_final(sh, data.data() + head + 32 * i);
        }
    };
    if (jobs > 1) parallel_for(jobs, body); else if (jobs == 1) body(0);
    hash_to_r_powers(data, count, out);
}

// one wire scalar -> 32 big-endian bytes of its canonical integer; false: the words are not below r
inline bool fr_encode_be(const uint64_t wire[4], uint8_t out[32]) {
    if (fr_geq_r(wire)) return false;
    fr_wire_to_be_bytes(wire, out);
    return true;
}
// one wire point -> 32 gnark-compressed bytes; the all-zero wire point -> 0x40 || zeros; false: a coordinate is not below p
inline bool g1_encode_be(const uint64_t xy[8], uint8_t out[32]) {
    const G1 p = g1_from_wire(xy);
    memset(out, 0, 32);
    if (p.inf) { out[0] = 0x40; return true; }
    if (geq_p(p.x) || geq_p(p.y)) return false;
    const Fq one_plain = {{1, 0, 0, 0}};
    const Fq x = mul(p.x, one_plain), y = mul(p.y, one_plain);                          // Montgomery -> canonical
    for (int i = 0; i < 4; ++i) put_u64be(out + 8 * i, x.l[3 - i]);
    const Fq ny = sub(FQ_P, y);
    bool larger = false;
    for (int i = 3; i >= 0; --i) if (y.l[i] != ny.l[i]) { larger = y.l[i] > ny.l[i]; break; }
    out[0] |= larger ? 0xC0 : 0x80;                                                     // x < p < 2^254 leaves the two top bits free
    return true;
}

}  // namespace kzg_host
