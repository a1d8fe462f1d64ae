// coset_item_stream.h — the message of one item digest of the coset transcript (host_fiat_shamir.h multiproof_r_powers_host), produced
// block by block from the item's WIRE data, for a lane that hashes it with dev_sha256.h (k_coset_item_digests of fsdevice.hip):
//
//     "KZGBN254_COSETITEM___V1_" || u64be(c) || u64be(k) || l x be32(canonical y_t) || ark-compressed proof          72 + 32 l bytes
//
// In big-endian words the message is a head of 10 words and then SLOTS of 8 words: slot t < l is value t (its canonical words, most
// significant first), slot l is the proof (x little-endian, so its words byte-swapped; 0x80 in the last byte when y > p - y, the
// all-zero wire point as 0x40 alone), slot l + 1 opens with the 0x80 pad byte and every later word is zero up to the bit length.  A block
// is words [16 b, 16 b + 16): block 0 = head + six words of slot 0, block b > 0 = the last two words of slot 2 b - 2, slot 2 b - 1,
// six words of slot 2 b.  Blocks are produced in order and every slot is converted once: the two words a block leaves over are the
// carry of the next.  Values go Montgomery -> canonical through fe_wire_to_canonical_words; a value >= r or a coordinate >= p sets
// `bad` (the host transcript does not validate such inputs; its bytes for them are not mirrored here, the caller falls back).
// Every function is KZG_HD: hipcc compiles it for the kernel, g++ for tests/test_fs_device_host.py.
#pragma once
#include "field29.h"
#include "dev_sha256.h"

namespace kzg {

struct CosetItemSrc {
    const uint32_t* ys;        // l x 8 wire words (16-byte aligned)
    const uint32_t* proof;     // 16 wire words x || y (16-byte aligned)
    uint64_t c, k;             // commitment row, coset index
    uint32_t l;
};

KZG_HD uint64_t coset_item_len(uint64_t l) { return 72 + 32 * l; }
KZG_HD uint32_t coset_item_blocks(uint64_t l) { return (uint32_t)sha256_n_blocks(coset_item_len(l)); }

KZG_HD void coset_item_load8(uint32_t w[8], const uint32_t* p) {
    const uint32_t* q = static_cast<const uint32_t*>(__builtin_assume_aligned(p, 16));
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = q[j];
}
// the 256-bit word string w is below the modulus of F
template <class F>
KZG_HD bool fe_words_below_modulus(const uint32_t w[8]) {
    Fe<F> t;
    fe_unpack(t, w);
    bool lt = false;
#pragma unroll
    for (int j = 0; j < NL; ++j) lt = t.l[j] < (int32_t)F::P[j] || (t.l[j] == (int32_t)F::P[j] && lt);
    return lt;
}

KZG_HD void coset_item_slot(uint32_t out[8], const CosetItemSrc& s, uint32_t t, uint32_t& bad) {
    if (t < s.l) {
        uint32_t w[8], c[8];
        coset_item_load8(w, s.ys + 8 * (size_t)t);
        bad |= fe_words_below_modulus<FrParams>(w) ? 0u : 1u;
        fe_wire_to_canonical_words<FrParams>(c, w);
#pragma unroll
        for (int j = 0; j < 8; ++j) out[j] = c[7 - j];
    } else if (t == s.l) {
        uint32_t x[8], y[8], cx[8], cy[8];
        coset_item_load8(x, s.proof);
        coset_item_load8(y, s.proof + 8);
        uint32_t any = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) any |= x[j] | y[j];
        bad |= (fe_words_below_modulus<FqParams>(x) && fe_words_below_modulus<FqParams>(y)) ? 0u : 1u;
        fe_wire_to_canonical_words<FqParams>(cx, x);
        fe_wire_to_canonical_words<FqParams>(cy, y);
        Fq d, yl;                                                       // 2 y - p: positive <=> y > p - y (p is odd: never zero)
        fe_unpack(yl, cy);
#pragma unroll
        for (int j = 0; j < NL; ++j) d.l[j] = 2 * yl.l[j] - (int32_t)FqParams::P[j];
        fe_norm(d);
        const uint32_t flag = any == 0 ? 0x40u : d.l[NL - 1] >= 0 ? 0x80u : 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) out[j] = any == 0 ? 0u : sha_bswap(cx[j]);
        out[7] |= flag;                                                 // byte 31 of the encoding: x < p < 2^254 leaves its two top bits free
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) out[j] = 0;
        if (t == s.l + 1) out[0] = 0x80000000u;
    }
}

// the 16 words of block b < coset_item_blocks(l), padding and length included.  Call with b = 0, 1, 2, .. in order: carry[2] is the state
KZG_HD void coset_item_block(uint32_t w[16], const CosetItemSrc& s, uint32_t b, uint32_t carry[2], uint32_t& bad) {
    uint32_t v[8];
    if (b == 0) {
        w[0] = 0x4b5a4742u; w[1] = 0x4e323534u; w[2] = 0x5f434f53u; w[3] = 0x45544954u; w[4] = 0x454d5f5fu; w[5] = 0x5f56315fu;   // the tag
        w[6] = (uint32_t)(s.c >> 32); w[7] = (uint32_t)s.c;
        w[8] = (uint32_t)(s.k >> 32); w[9] = (uint32_t)s.k;
    } else {
        w[0] = carry[0]; w[1] = carry[1];
        coset_item_slot(v, s, 2 * b - 1, bad);
#pragma unroll
        for (int j = 0; j < 8; ++j) w[2 + j] = v[j];
    }
    coset_item_slot(v, s, 2 * b, bad);
#pragma unroll
    for (int j = 0; j < 6; ++j) w[10 + j] = v[j];
    carry[0] = v[6]; carry[1] = v[7];
    if (b + 1 == coset_item_blocks(s.l)) {                              // the 0x80 byte is in place (slot l + 1); both words are zero before
        const uint64_t len = coset_item_len(s.l);
        w[14] = (uint32_t)(len >> 29);
        w[15] = (uint32_t)(len << 3);
    }
}

// ---------------------------------------------------------------------------------------------
// The second producer: the same message from the item's SERIALIZED form (cosetbytes.hip k_coset_item_digests_bytes) -- values as 32
// big-endian bytes each, the proof as 32 gnark-compressed bytes, both as the words a little-endian load of them leaves.  For inputs
// that decode (g1_decode.h: canonical x, canonical values) be32(y_t) is the value's bytes as they are, and the ark-compressed proof is
// the gnark bytes reversed with the flag bits remapped (0b10 -> 0, 0b11 -> 0x80, 0b01 -> 0x40, 0b00 -> 0xC0; host_coset_bytes.h
// gnark_to_ark): no field arithmetic, nothing to refuse here -- the decode kernels refuse, and then no weight is used.
// ---------------------------------------------------------------------------------------------
struct CosetItemBytesSrc {
    const uint32_t* ys;        // l x 8 words of bytes (16-byte aligned)
    const uint32_t* proof;     // 8 words of bytes (16-byte aligned)
    uint64_t c, k;
    uint32_t l;
};

KZG_HD void coset_item_bytes_slot(uint32_t out[8], const CosetItemBytesSrc& s, uint32_t t) {
    if (t < s.l) {
        uint32_t w[8];
        coset_item_load8(w, s.ys + 8 * (size_t)t);
#pragma unroll
        for (int j = 0; j < 8; ++j) out[j] = sha_bswap(w[j]);           // message bytes in order: big-endian word j = the loaded word j, swapped
    } else if (t == s.l) {
        uint32_t w[8];
        coset_item_load8(w, s.proof);
#pragma unroll
        for (int j = 0; j < 8; ++j) out[j] = w[7 - j];                  // the reversed bytes as big-endian words: the loaded words in reverse order, unswapped
        const uint32_t f = (w[0] >> 6) & 3u;                            // the top two bits of gnark's byte 0 = ark's byte 31 = the low byte of out[7]
        const uint32_t flag = f == 0u ? 0xC0u : f == 1u ? 0x40u : f == 2u ? 0u : 0x80u;
        out[7] = (out[7] & ~0xC0u) | flag;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) out[j] = 0;
        if (t == s.l + 1) out[0] = 0x80000000u;
    }
}

// the 16 words of block b, as coset_item_block above
KZG_HD void coset_item_bytes_block(uint32_t w[16], const CosetItemBytesSrc& s, uint32_t b, uint32_t carry[2]) {
    uint32_t v[8];
    if (b == 0) {
        w[0] = 0x4b5a4742u; w[1] = 0x4e323534u; w[2] = 0x5f434f53u; w[3] = 0x45544954u; w[4] = 0x454d5f5fu; w[5] = 0x5f56315fu;   // the tag
        w[6] = (uint32_t)(s.c >> 32); w[7] = (uint32_t)s.c;
        w[8] = (uint32_t)(s.k >> 32); w[9] = (uint32_t)s.k;
    } else {
        w[0] = carry[0]; w[1] = carry[1];
        coset_item_bytes_slot(v, s, 2 * b - 1);
#pragma unroll
        for (int j = 0; j < 8; ++j) w[2 + j] = v[j];
    }
    coset_item_bytes_slot(v, s, 2 * b);
#pragma unroll
    for (int j = 0; j < 6; ++j) w[10 + j] = v[j];
    carry[0] = v[6]; carry[1] = v[7];
    if (b + 1 == coset_item_blocks(s.l)) {
        const uint64_t len = coset_item_len(s.l);
        w[14] = (uint32_t)(len >> 29);
        w[15] = (uint32_t)(len << 3);
    }
}

}  // namespace kzg
