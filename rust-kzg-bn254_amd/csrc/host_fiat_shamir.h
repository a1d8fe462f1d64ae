// host_fiat_shamir.h — the Fiat-Shamir codec of the library, one of each piece: the byte encoders, digest -> Fr, the challenge of
// helpers::compute_challenge (primitives/src/helpers.rs:411-472), and the two random-linear-combination transcripts (the reference's
// batch verifier, verifier/src/batch.rs:76-168, and this library's own for FK20 coset proofs).  Pure host code (no HIP, no engine.h):
// also compiled by g++ for tests/test_fiat_shamir_host.py.  The two transcripts fan their rows out through a parallel-for handed in by
// the caller (the library: kzg::host_parallel_for).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <vector>
#include "host_fr.h"
#include "host_pairing.h"
#include "host_sha256.h"
#include "host_transcript.h"

namespace kzg_host {

using ParallelFor = void (*)(size_t n, const std::function<void(size_t)>& job);   // job(i) for i < n, in any order, on any threads

const char RC_BATCH_DOMAIN[] = "EIGENDA_RCKZGBATCH___V1_";       // primitives/src/consts.rs:11 (24 bytes)
const char COSET_ITEM_DOMAIN[] = "KZGBN254_COSETITEM___V1_";     // 24 bytes each; this library's own transcript (the reference has no coset proofs)
const char COSET_BATCH_DOMAIN[] = "KZGBN254_COSETBATCH__V1_";
const char COSET_MIXED_DOMAIN[] = "KZGBN254_COSETMIXED__V1_";    // the batch level of a batch of mixed shapes (the item level is COSET_ITEM_DOMAIN's)
const char HEADER_ITEM_DOMAIN[] = "KZGBN254_HEADERITEM__V1_";    // 24 bytes each; this library's own transcript for batches of blob headers
const char HEADER_BATCH_DOMAIN[] = "KZGBN254_HEADERBATCH_V1_";

inline size_t next_pow2(size_t x) { size_t p = 1; while (p < x) p <<= 1; return p; }           // next_power_of_two(0) == 1
inline size_t blob_padded_len(size_t len) { return next_pow2((len + 31) / 32); }               // elements of Blob::to_polynomial_eval_form
inline void put_u64be(uint8_t* p, uint64_t v) { for (int b = 0; b < 8; ++b) p[b] = (uint8_t)(v >> (8 * (7 - b))); }
inline void fr_wire_to_be_bytes(const uint64_t wire[4], uint8_t out[32]) {
    uint64_t k[4];
    fr_wire_to_canonical(wire, k);
    for (int i = 0; i < 4; ++i) put_u64be(out + 8 * i, k[3 - i]);
}
inline void digest_to_fr_wire(const uint8_t dig[32], uint64_t out[4]) {            // hash_to_field_element (helpers.rs:382-390)
    uint64_t w[4];
    for (int i = 0; i < 4; ++i) { uint64_t v = 0; for (int b = 0; b < 8; ++b) v = (v << 8) | dig[8 * (3 - i) + b]; w[i] = v; }
    while (fr_geq_r(w)) fr_sub_r(w);                                                // Fr::from_be_bytes_mod_order
    fr_mul(w, FR_R2, out);                                                          // canonical -> Montgomery
}
// ark-serialize compressed G1Affine (helpers.rs:456-459): x little-endian, bit 7 of the last byte = y is the larger root, bit 6 = infinity
inline void g1_serialize_compressed_ark(const G1& p, uint8_t out[32]) {
    memset(out, 0, 32);
    if (p.inf) { out[31] = 0x40; return; }
    Fq one_plain = {{1, 0, 0, 0}};
    Fq x = mul(p.x, one_plain), y = mul(p.y, one_plain);                             // Montgomery -> canonical
    memcpy(out, x.l, 32);                                                            // little-endian host
    Fq ny = sub(FQ_P, y);                                                            // -y (y != 0 on this curve)
    bool larger = false;
    for (int i = 3; i >= 0; --i) if (y.l[i] != ny.l[i]) { larger = y.l[i] > ny.l[i]; break; }
    if (larger) out[31] |= 0x80;
}

// Absorbs  tag || u64be(n) || n x 32 bytes, the evaluations of Blob::to_polynomial_eval_form in to_byte_array form: every
// 32-byte big-endian chunk of the blob reduced mod r (helpers.rs:40-57 -> :80-119), zero elements up to the next power of two.
// Canonical chunks (the normal case) are hashed straight from the caller's buffer.
inline void challenge_absorb_prefix(Sha256& sh, const uint8_t* blob, size_t len, size_t n_padded) {
    TranscriptPrefix gen(blob, len, n_padded);                                       // host_transcript.h
    sha256_absorb(sh, gen);
}
inline void challenge_finish(Sha256& sh, const G1& commitment, uint64_t out_z_mont[4]) {
    uint8_t cb[32], dig[32];
    g1_serialize_compressed_ark(commitment, cb);
    sha256_update(sh, cb, 32);
    sha256_final(sh, dig);
    digest_to_fr_wire(dig, out_z_mont);
}

// helpers::compute_powers (helpers.rs:298-313): out[i] = r^i for i < n, wire form
inline void powers_of(const uint64_t r[4], size_t n, uint64_t* out) {
    uint64_t cur[4];
    fr_one(cur);
    for (size_t i = 0; i < n; ++i) { memcpy(out + 4 * i, cur, 32); fr_mul(cur, r, cur); }
}
// the tail of both transcripts: r = hash_to_field_element(data), then the n powers of r
inline void hash_to_r(const std::vector<uint8_t>& data, uint64_t r[4]) {
    Sha256 sh;
    sha256_init(sh);
    sha256_update(sh, data.data(), data.size());
    uint8_t dig[32];
    sha256_final(sh, dig);
    digest_to_fr_wire(dig, r);
}
inline void hash_to_r_powers(const std::vector<uint8_t>& data, size_t n, uint64_t* out) {
    uint64_t r[4];
    hash_to_r(data, r);
    powers_of(r, n, out);
}

// batch.rs:76-168 on the host: 40 + 8 n + 128 n transcript bytes, one SHA-256, n - 1 field multiplications
inline void r_powers_host(const uint64_t* commitments, const uint64_t* zs, const uint64_t* ys, const uint64_t* proofs, const uint64_t* lens_elems,
                          size_t n, uint64_t* out, ParallelFor parallel_for) {
    std::vector<uint8_t> data(40 + n * 8 + n * 128, 0);
    memcpy(data.data(), RC_BATCH_DOMAIN, 24);                                          // bytes 24..31 stay zero (batch.rs:107-112)
    put_u64be(data.data() + 32, (uint64_t)n);
    for (size_t i = 0; i < n; ++i) put_u64be(data.data() + 40 + 8 * i, lens_elems[i]);
    uint8_t* rows = data.data() + 40 + 8 * n;
    const size_t per = 64, jobs = (n + per - 1) / per;
    parallel_for(jobs, [&](size_t j) {
        for (size_t i = j * per; i < std::min(n, (j + 1) * per); ++i) {
            uint8_t* p = rows + 128 * i;
            g1_serialize_compressed_ark(g1_from_wire(commitments + 8 * i), p);
            fr_wire_to_be_bytes(zs + 4 * i, p + 32);
            fr_wire_to_be_bytes(ys + 4 * i, p + 64);
            g1_serialize_compressed_ark(g1_from_wire(proofs + 8 * i), p + 96);
        }
    });
    hash_to_r_powers(data, n, out);
}

// The batch level of the coset transcript: tag, sizes and commitments filled in, room for the `count` item digests from coset_batch_head() on
inline size_t coset_batch_head(size_t n_commitments) { return 24 + 32 + 32 * n_commitments; }
inline std::vector<uint8_t> coset_batch_transcript(const uint64_t* commitments, size_t n_commitments, size_t count, size_t n, size_t l) {
    std::vector<uint8_t> data(coset_batch_head(n_commitments) + 32 * count, 0);
    memcpy(data.data(), COSET_BATCH_DOMAIN, 24);
    put_u64be(data.data() + 24, (uint64_t)n);
    put_u64be(data.data() + 32, (uint64_t)l);
    put_u64be(data.data() + 40, (uint64_t)n_commitments);
    put_u64be(data.data() + 48, (uint64_t)count);
    for (size_t c = 0; c < n_commitments; ++c) g1_serialize_compressed_ark(g1_from_wire(commitments + 8 * c), data.data() + 56 + 32 * c);
    return data;
}
// Where the item digests of a batch are hashed (kzg_ctx_set_transcript_device: mode 1 host, 2 device).  Automatic (0) takes the device only
// inside the envelope that was MEASURED to win (profiles/fs_device.md): at least 4 096 items, chunks of at most 64 values, at least 2 MiB of
// values.  A lane hashes its item as one dependent chain of 2 + l / 2 blocks, so few long items (count small, l large) are the shape a lane
// per stream does not fit, and batches of 256 items lose to the two extra round trips at every chunk length: both stay on the host pool.
constexpr size_t COSET_DEVICE_MIN_COUNT = 4096, COSET_DEVICE_MAX_CHUNK = 64, COSET_DEVICE_MIN_BYTES = (size_t)2 << 20;
inline bool coset_transcript_on_device(int mode, size_t count, size_t l) {
    if (mode != 0) return mode == 2;
    return count >= COSET_DEVICE_MIN_COUNT && l <= COSET_DEVICE_MAX_CHUNK && count * l * 32 >= COSET_DEVICE_MIN_BYTES;
}
// Two levels: one SHA-256 per item over its index pair, its l values and its proof (host pool), one over the header, the commitments and the digests
// (fsdevice.hip computes the same item digests on the device, one lane per item, from coset_item_stream.h)
inline void multiproof_r_powers_host(const uint64_t* commitments, size_t n_commitments, const uint64_t* commitment_indices, const uint64_t* coset_indices,
                                     const uint64_t* ys, const uint64_t* proofs, size_t count, size_t n, size_t l, uint64_t* out, ParallelFor parallel_for) {
    const size_t head = coset_batch_head(n_commitments);
    std::vector<uint8_t> data = coset_batch_transcript(commitments, n_commitments, count, n, l);
    const size_t per = std::max<size_t>(1, 1024 / l), jobs = (count + per - 1) / per;
    auto body = [&](size_t j) {
        std::vector<uint8_t> item(24 + 16 + 32 * l + 32);
        memcpy(item.data(), COSET_ITEM_DOMAIN, 24);
        for (size_t i = j * per; i < std::min(count, (j + 1) * per); ++i) {
            put_u64be(item.data() + 24, commitment_indices[i]);
            put_u64be(item.data() + 32, coset_indices[i]);
            for (size_t t = 0; t < l; ++t) fr_wire_to_be_bytes(ys + 4 * (i * l + t), item.data() + 40 + 32 * t);
            g1_serialize_compressed_ark(g1_from_wire(proofs + 8 * i), item.data() + 40 + 32 * l);
            Sha256 sh;
            sha256_init(sh);
            sha256_update(sh, item.data(), item.size());
            sha256_final(sh, data.data() + head + 32 * i);
        }
    };
    if (jobs > 1) parallel_for(jobs, body); else if (jobs == 1) body(0);
    hash_to_r_powers(data, count, out);
}

// The transcript of a batch of MIXED shapes (kzg_compute_multiproof_r_powers_mixed): class s is (n_s, l_s), item i has class s_i and its own
// l_{s_i} values at ys + 4 value_offsets[i] (ragged, the caller's order).  The item digest is the one above, over the item's own values;
// the batch level is COSET_MIXED_DOMAIN || u64be(n_classes) || n_classes x (u64be(n_s) || u64be(l_s)) || u64be(n_commitments) ||
// u64be(count) || count x u64be(s_i) || the commitments || the digests.
inline void multiproof_r_powers_mixed_host(const uint64_t* commitments, size_t n_commitments, const uint64_t* commitment_indices, const uint64_t* class_n,
                                           const uint64_t* class_chunk_len, size_t n_classes, const uint64_t* class_indices, const uint64_t* coset_indices,
                                           const uint64_t* ys, const uint32_t* value_offsets, const uint64_t* proofs, size_t count, uint64_t* out,
                                           ParallelFor parallel_for) {
    const size_t head = 24 + 8 + 16 * n_classes + 16 + 8 * count + 32 * n_commitments;
    std::vector<uint8_t> data(head + 32 * count, 0);
    uint8_t* p = data.data();
    memcpy(p, COSET_MIXED_DOMAIN, 24); p += 24;
    put_u64be(p, (uint64_t)n_classes); p += 8;
    for (size_t s = 0; s < n_classes; ++s) { put_u64be(p, class_n[s]); put_u64be(p + 8, class_chunk_len[s]); p += 16; }
    put_u64be(p, (uint64_t)n_commitments); put_u64be(p + 8, (uint64_t)count); p += 16;
    for (size_t i = 0; i < count; ++i) { put_u64be(p, class_indices[i]); p += 8; }
    for (size_t c = 0; c < n_commitments; ++c) { g1_serialize_compressed_ark(g1_from_wire(commitments + 8 * c), p); p += 32; }
    const size_t per = 16, jobs = (count + per - 1) / per;
    auto body = [&](size_t j) {
        std::vector<uint8_t> item;
        for (size_t i = j * per; i < std::min(count, (j + 1) * per); ++i) {
            const size_t l = (size_t)class_chunk_len[class_indices[i]];
            item.resize(24 + 16 + 32 * l + 32);
            memcpy(item.data(), COSET_ITEM_DOMAIN, 24);
            put_u64be(item.data() + 24, commitment_indices[i]);
            put_u64be(item.data() + 32, coset_indices[i]);
            for (size_t t = 0; t < l; ++t) fr_wire_to_be_bytes(ys + 4 * ((size_t)value_offsets[i] + t), item.data() + 40 + 32 * t);
            g1_serialize_compressed_ark(g1_from_wire(proofs + 8 * i), item.data() + 40 + 32 * l);
            Sha256 sh;
            sha256_init(sh);
            sha256_update(sh, item.data(), item.size());
            sha256_final(sh, data.data() + head + 32 * i);
        }
    };
    if (jobs > 1) parallel_for(jobs, body); else if (jobs == 1) body(0);
    hash_to_r_powers(data, count, out);
}

// G2 point as 128 bytes: be32(x.c0) || be32(x.c1) || be32(y.c0) || be32(y.c1) on canonical integers; the identity is 128 zero bytes
inline void g2_serialize_be(const G2& p, uint8_t out[128]) {
    memset(out, 0, 128);
    if (p.inf) return;
    const Fq one_plain = {{1, 0, 0, 0}};
    const Fq* c[4] = {&p.x.c0, &p.x.c1, &p.y.c0, &p.y.c1};
    for (int q = 0; q < 4; ++q) {
        const Fq v = mul(*c[q], one_plain);                                             // Montgomery -> canonical
        for (int i = 0; i < 4; ++i) put_u64be(out + 32 * q + 8 * i, v.l[3 - i]);
    }
}
// The weights of a batch of blob headers (kzg_verify_length_proof_batch): count + 1 values below 2^128, wire form.  Two levels like
// the coset transcript: d_i = SHA-256(item tag || u64be(len_i) || C_i || C2_i || pi2_i) on the host pool, seed = SHA-256(batch tag ||
// u64be(count) || u64be(n_shifts) || n_shifts x (u64be(len) || shift) || d_0 .. d_(count-1)), and weight j = the first 16 bytes, read
// big-endian, of SHA-256(seed || u64be(j)); j = count is rho, the weight between the two equations.
// The pieces are functions of their own for the entries that hash the items elsewhere (headerbytes.hip, from serialized headers): the item
// message, the batch level with tag, sizes and shifts filled in and room for the `count` item digests from header_batch_head() on, the tail.
constexpr size_t HEADER_ITEM_BYTES = 24 + 8 + 32 + 128 + 128;
inline void header_item_message(uint64_t claimed_len, const uint64_t commitment[8], const uint64_t length_commitment[16], const uint64_t length_proof[16],
                                uint8_t item[HEADER_ITEM_BYTES]) {
    memcpy(item, HEADER_ITEM_DOMAIN, 24);
    put_u64be(item + 24, claimed_len);
    g1_serialize_compressed_ark(g1_from_wire(commitment), item + 32);
    g2_serialize_be(g2_from_wire(length_commitment), item + 64);
    g2_serialize_be(g2_from_wire(length_proof), item + 192);
}
inline size_t header_batch_head(size_t n_shifts) { return 24 + 16 + 40 * n_shifts; }
inline std::vector<uint8_t> header_batch_transcript(size_t count, const uint64_t* shift_lens, const uint64_t* shifts, size_t n_shifts) {
    std::vector<uint8_t> data(header_batch_head(n_shifts) + 32 * count, 0);
    memcpy(data.data(), HEADER_BATCH_DOMAIN, 24);
    put_u64be(data.data() + 24, (uint64_t)count);
    put_u64be(data.data() + 32, (uint64_t)n_shifts);
    for (size_t g = 0; g < n_shifts; ++g) {
        put_u64be(data.data() + 40 + 40 * g, shift_lens[g]);
        g1_serialize_compressed_ark(g1_from_wire(shifts + 8 * g), data.data() + 48 + 40 * g);
    }
    return data;
}
// the tail: the seed over the complete batch transcript, then the count + 1 one-block weight hashes
inline void header_weights_from_transcript(const std::vector<uint8_t>& data, size_t count, uint64_t* out, ParallelFor parallel_for) {
    uint8_t seed[40];
    {
        Sha256 sh;
        sha256_init(sh);
        sha256_update(sh, data.data(), data.size());
        sha256_final(sh, seed);
    }
    const size_t wjobs = (count + 1 + 255) / 256;
    auto wbody = [&](size_t j) {
        uint8_t msg[40], dig[32];
        memcpy(msg, seed, 32);
        for (size_t i = j * 256; i < std::min(count + 1, (j + 1) * 256); ++i) {
            put_u64be(msg + 32, (uint64_t)i);
            Sha256 sh;
            sha256_init(sh);
            sha256_update(sh, msg, 40);
            sha256_final(sh, dig);
            uint64_t w[4] = {0, 0, 0, 0};
            for (int b = 0; b < 8; ++b) { w[1] = (w[1] << 8) | dig[b]; w[0] = (w[0] << 8) | dig[8 + b]; }
            fr_mul(w, FR_R2, out + 4 * i);                                              // canonical (below 2^128 < r) -> Montgomery
        }
    };
    if (wjobs > 1) parallel_for(wjobs, wbody); else wbody(0);
}
inline void header_batch_weights_host(const uint64_t* commitments, const uint64_t* length_commitments, const uint64_t* length_proofs,
                                      const uint64_t* claimed_lens, size_t count, const uint64_t* shift_lens, const uint64_t* shifts, size_t n_shifts,
                                      uint64_t* out, ParallelFor parallel_for) {
    const size_t head = header_batch_head(n_shifts);
    std::vector<uint8_t> data = header_batch_transcript(count, shift_lens, shifts, n_shifts);
    const size_t per = 64, jobs = (count + per - 1) / per;
    auto body = [&](size_t j) {
        uint8_t item[HEADER_ITEM_BYTES];
        for (size_t i = j * per; i < std::min(count, (j + 1) * per); ++i) {
            header_item_message(claimed_lens[i], commitments + 8 * i, length_commitments + 16 * i, length_proofs + 16 * i, item);
            Sha256 sh;
            sha256_init(sh);
            sha256_update(sh, item, sizeof item);
            sha256_final(sh, data.data() + head + 32 * i);
        }
    };
    if (jobs > 1) parallel_for(jobs, body); else if (jobs == 1) body(0);
    header_weights_from_transcript(data, count, out, parallel_for);
}

}  // namespace kzg_host
