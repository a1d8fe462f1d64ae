// dev_sha256.h — SHA-256 for code that runs on the device and on the host alike: the block function over a 16-word message window and
// an 8-word state, the initial state, and the padding / length tail of a message whose length is known before its first block.
// One hash stream is sequential (host_sha256.h keeps the host's: SHA extensions, incremental interface); this header is for MANY
// independent streams of one length, a lane per stream (fsdevice.hip).  Plain C++ on 32-bit words: fully unrolled, the schedule kept as a
// rolling window of 16 words with every index a literal, so that on the device the state and the window live in registers and nothing is
// indexed dynamically.  No inline assembly; the rotations are the align-bit builtin on the device and two shifts on the host.
// Every function is KZG_HD: hipcc compiles it for the kernels, g++ for tests/test_fs_device_host.py.
#pragma once
#include <cstddef>
#include <cstdint>

#if !defined(KZG_HD)               // field29.h's definitions, token for token
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KZG_HD __host__ __device__ __forceinline__
#define KZG_HD_NOINLINE __host__ __device__ __noinline__ inline
#else
#define KZG_HD inline
#define KZG_HD_NOINLINE inline
#endif
#endif

namespace kzg {

template <int N>
KZG_HD uint32_t sha_rotr(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(x, x, N);               // the low word of (x : x) >> N
#else
    return (x >> N) | (x << (32 - N));
#endif
}
KZG_HD uint32_t sha_bswap(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }
KZG_HD uint32_t sha_big_sigma0(uint32_t a) { return sha_rotr<2>(a) ^ sha_rotr<13>(a) ^ sha_rotr<22>(a); }
KZG_HD uint32_t sha_big_sigma1(uint32_t e) { return sha_rotr<6>(e) ^ sha_rotr<11>(e) ^ sha_rotr<25>(e); }
KZG_HD uint32_t sha_small_sigma0(uint32_t x) { return sha_rotr<7>(x) ^ sha_rotr<18>(x) ^ (x >> 3); }
KZG_HD uint32_t sha_small_sigma1(uint32_t x) { return sha_rotr<17>(x) ^ sha_rotr<19>(x) ^ (x >> 10); }
KZG_HD uint32_t sha_ch(uint32_t e, uint32_t f, uint32_t g) { return (e & f) | (~e & g); }
KZG_HD uint32_t sha_maj(uint32_t a, uint32_t b, uint32_t c) { return (a & b) | (c & (a | b)); }

KZG_HD void sha256_init_state(uint32_t st[8]) {
    st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
    st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}

// one round with the registers named by position; the caller rotates the names instead of the values
#define KZG_SHA_RND(a, b, c, d, e, f, g, h, kw)                                                  \
    do {                                                                                         \
        const uint32_t t1_ = (h) + sha_big_sigma1(e) + sha_ch(e, f, g) + (kw);                   \
        const uint32_t t2_ = sha_big_sigma0(a) + sha_maj(a, b, c);                               \
        (d) += t1_;                                                                              \
        (h) = t1_ + t2_;                                                                         \
    } while (0)
// message word i: the window itself for i < 16, then w[i mod 16] = w[i - 16] + s0(w[i - 15]) + w[i - 7] + s1(w[i - 2]) in place
#define KZG_SHA_W_FIRST(i) w[(i)]
#define KZG_SHA_W_NEXT(i) (w[(i) & 15] += sha_small_sigma1(w[((i) - 2) & 15]) + w[((i) - 7) & 15] + sha_small_sigma0(w[((i) - 15) & 15]))
#define KZG_SHA_8(W, i, k0, k1, k2, k3, k4, k5, k6, k7)     \
    KZG_SHA_RND(a, b, c, d, e, f, g, h, k0 + W((i) + 0));  \
    KZG_SHA_RND(h, a, b, c, d, e, f, g, k1 + W((i) + 1));  \
    KZG_SHA_RND(g, h, a, b, c, d, e, f, k2 + W((i) + 2));  \
    KZG_SHA_RND(f, g, h, a, b, c, d, e, k3 + W((i) + 3));  \
    KZG_SHA_RND(e, f, g, h, a, b, c, d, k4 + W((i) + 4));  \
    KZG_SHA_RND(d, e, f, g, h, a, b, c, k5 + W((i) + 5));  \
    KZG_SHA_RND(c, d, e, f, g, h, a, b, k6 + W((i) + 6));  \
    KZG_SHA_RND(b, c, d, e, f, g, h, a, k7 + W((i) + 7))

// st <- compress(st, w): w = the 16 big-endian words of one block; it is the rolling schedule afterwards (overwritten)
KZG_HD void sha256_compress(uint32_t st[8], uint32_t w[16]) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    KZG_SHA_8(KZG_SHA_W_FIRST, 0, 0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u);
    KZG_SHA_8(KZG_SHA_W_FIRST, 8, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u);
    KZG_SHA_8(KZG_SHA_W_NEXT, 16, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau);
    KZG_SHA_8(KZG_SHA_W_NEXT, 24, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u);
    KZG_SHA_8(KZG_SHA_W_NEXT, 32, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u);
    KZG_SHA_8(KZG_SHA_W_NEXT, 40, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u);
    KZG_SHA_8(KZG_SHA_W_NEXT, 48, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u);
    KZG_SHA_8(KZG_SHA_W_NEXT, 56, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u);
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}
#undef KZG_SHA_8
#undef KZG_SHA_W_NEXT
#undef KZG_SHA_W_FIRST
#undef KZG_SHA_RND

// ---- messages of known length --------------------------------------------------------------------------------------------------
// A message of len bytes is sha256_n_blocks(len) blocks: its bytes, one 0x80 byte, zeros, and the bit length in the last 8 bytes.
KZG_HD uint64_t sha256_n_blocks(uint64_t len) { return (len + 9 + 63) / 64; }
// w = the words of block b of the message with every byte from `len` on zero -> the block as it is hashed: the 0x80 byte when byte
// `len` lies in this block, the bit length when this is the last one.  (Selects over literal indices, no indexed store.)
KZG_HD void sha256_pad_block(uint32_t w[16], uint64_t len, uint64_t b) {
    const bool here = (len >> 6) == b;
    const uint32_t word = (uint32_t)(len & 63) >> 2, bit = 0x80u << (24 - 8 * ((uint32_t)len & 3));
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) w[j] |= (here && j == word) ? bit : 0u;
    if (b + 1 == sha256_n_blocks(len)) {
        w[14] = (uint32_t)(len >> 29);
        w[15] = (uint32_t)(len << 3);
    }
}
// the same block read from a byte string at any alignment: msg[0 .. len)
KZG_HD void sha256_message_block(uint32_t w[16], const uint8_t* msg, uint64_t len, uint64_t b) {
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const uint64_t at = 64 * b + 4 * j + q;
            v = (v << 8) | (at < len ? (uint32_t)msg[at] : 0u);
        }
        w[j] = v;
    }
    sha256_pad_block(w, len, b);
}
// the state as the 32 digest bytes, in little-endian words (so that a word store writes the bytes in order)
KZG_HD void sha256_digest_le_words(uint32_t out[8], const uint32_t st[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = sha_bswap(st[j]);
}

}  // namespace kzg
