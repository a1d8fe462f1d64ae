// tests/hostcheck/fsdevcheck.cpp — TEST-ONLY: csrc/dev_sha256.h and csrc/coset_item_stream.h, the code the hashing kernels of
// csrc/fsdevice.hip run one lane per message, compiled by g++ (no GPU, no library).  Two builds of this one file:
//   * a shared object whose C entry points tests/test_fs_device_host.py compares with hashlib and with the item bytes of
//     verifier.compute_multiproof_r_powers_py;
//   * -DFSDEVCHECK_MAIN: a stand-alone program (for -fsanitize=address,undefined) that compares the same functions with the host codec of
//     csrc/host_fiat_shamir.h and csrc/host_sha256.h and prints "fsdevcheck ok"; a failed check prints its line and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "coset_item_stream.h"
#include "host_fiat_shamir.h"

using namespace kzg;

static void digest_bytes(const uint32_t st[8], uint8_t out[32]) {
    uint32_t o[8];
    sha256_digest_le_words(o, st);
    memcpy(out, o, 32);                                                      // little-endian host, as the device
}

extern "C" {
// SHA-256 of msg[0 .. len) through the block function and the known-length tail
void fsdev_sha256(const uint8_t* msg, size_t len, uint8_t out[32]) {
    uint32_t st[8], w[16];
    sha256_init_state(st);
    for (uint64_t b = 0; b < sha256_n_blocks(len); ++b) {
        sha256_message_block(w, msg, len, b);
        sha256_compress(st, w);
    }
    digest_bytes(st, out);
}
int fsdev_on_device(int mode, size_t count, size_t l) { return kzg_host::coset_transcript_on_device(mode, count, l) ? 1 : 0; }
size_t fsdev_item_blocks(size_t l) { return coset_item_blocks(l); }
// the padded message of one item as the kernel's lane produces it, 64 coset_item_blocks(l) bytes, and its digest; returns the flag
uint32_t fsdev_item(const uint64_t* ys, const uint64_t* proof, uint64_t c, uint64_t k, size_t l, uint8_t* out_stream, uint8_t out_digest[32]) {
    CosetItemSrc src{reinterpret_cast<const uint32_t*>(ys), reinterpret_cast<const uint32_t*>(proof), c, k, (uint32_t)l};
    uint32_t st[8], w[16], carry[2] = {0, 0}, bad = 0;
    sha256_init_state(st);
    for (uint32_t b = 0; b < coset_item_blocks(l); ++b) {
        coset_item_block(w, src, b, carry, bad);
        for (int j = 0; j < 16; ++j) for (int q = 0; q < 4; ++q) out_stream[64 * (size_t)b + 4 * j + q] = (uint8_t)(w[j] >> (24 - 8 * q));
        sha256_compress(st, w);
    }
    digest_bytes(st, out_digest);
    return bad;
}
}

#if defined(FSDEVCHECK_MAIN)
#define CHECK(cond) do { if (!(cond)) { printf("fsdevcheck: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

int main() {
    using namespace kzg_host;
    // 1. digests at the padding boundaries against the host's SHA-256
    const size_t lens[] = {0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 2120};
    for (size_t len : lens) {
        std::vector<uint8_t> msg(len);                                       // (exactly len bytes: a read past the end is the sanitizer's to find)
        for (auto& v : msg) v = (uint8_t)rng();
        uint8_t got[32], want[32];
        fsdev_sha256(msg.data(), len, got);
        Sha256 sh;
        sha256_init(sh);
        sha256_update(sh, msg.data(), len);
        sha256_final(sh, want);
        CHECK(memcmp(got, want, 32) == 0);
    }
    // 2. item streams against the host codec: the identity proof, a point and its negative, values 0, 1 and r - 1
    uint64_t gw[8];                                                          // the generator (1, 2) in wire form
    const kzg_host::Fq two = add(FQ_ONE, FQ_ONE);
    memcpy(gw, FQ_ONE.l, 32);
    memcpy(gw + 4, two.l, 32);
    const G1 g = g1_from_wire(gw);
    const G1 pts[3] = {g1_from_wire(std::vector<uint64_t>(8, 0).data()), g1_add(g, g1_add(g, g)), g1_neg(g1_add(g, g1_add(g, g)))};
    int flags_seen = 0;
    for (size_t l : {(size_t)1, (size_t)2, (size_t)16, (size_t)64}) {
        for (int pi = 0; pi < 3; ++pi) {
            std::vector<uint64_t> ys(4 * l), proof(8, 0);
            for (size_t t = 0; t < l; ++t) {
                uint64_t v[4] = {rng(), rng(), rng(), rng() >> 3};             // < 2^253 < r
                if (t % 3 == 0) { const uint64_t small[4] = {(uint64_t)(t % 2), 0, 0, 0}; memcpy(v, small, 32); }
                if (t == l - 1) { memcpy(v, FR_MODULUS_WORDS, 32); v[0] -= 1; }
                fr_mul(v, FR_R2, ys.data() + 4 * t);                         // canonical -> wire
            }
            if (!pts[pi].inf) { memcpy(proof.data(), pts[pi].x.l, 32); memcpy(proof.data() + 4, pts[pi].y.l, 32); }
            const uint64_t c = 0x0102030405060708ULL + pi, k = rng();
            std::vector<uint8_t> want(24 + 16 + 32 * l + 32), stream(64 * fsdev_item_blocks(l));
            memcpy(want.data(), COSET_ITEM_DOMAIN, 24);
            put_u64be(want.data() + 24, c);
            put_u64be(want.data() + 32, k);
            for (size_t t = 0; t < l; ++t) fr_wire_to_be_bytes(ys.data() + 4 * t, want.data() + 40 + 32 * t);
            g1_serialize_compressed_ark(g1_from_wire(proof.data()), want.data() + 40 + 32 * l);
            flags_seen |= want.back() & 0xC0 ? want.back() & 0xC0 : 1;
            uint8_t got[32], dig[32];
            CHECK(fsdev_item(ys.data(), proof.data(), c, k, l, stream.data(), got) == 0);
            CHECK(stream.size() >= want.size() + 9 && memcmp(stream.data(), want.data(), want.size()) == 0);
            Sha256 sh;
            sha256_init(sh);
            sha256_update(sh, want.data(), want.size());
            sha256_final(sh, dig);
            CHECK(memcmp(got, dig, 32) == 0);
        }
    }
    CHECK(flags_seen == (0x40 | 0x80 | 1));                                  // the identity, the larger root and the smaller root all appeared
    // 3. the flag: a value equal to r, a coordinate equal to p
    {
        std::vector<uint64_t> ys(4), proof(8, 0);
        std::vector<uint8_t> stream(64 * fsdev_item_blocks(1));
        uint8_t dig[32];
        memcpy(ys.data(), FR_MODULUS_WORDS, 32);
        CHECK(fsdev_item(ys.data(), proof.data(), 0, 0, 1, stream.data(), dig) == 1);
        ys[0] -= 1;
        CHECK(fsdev_item(ys.data(), proof.data(), 0, 0, 1, stream.data(), dig) == 0);
        memcpy(proof.data() + 4, FQ_P.l, 32);
        CHECK(fsdev_item(ys.data(), proof.data(), 0, 0, 1, stream.data(), dig) == 1);
    }
    printf("fsdevcheck ok\n");
    return 0;
}
#endif
