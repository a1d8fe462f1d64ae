// tests/hostcheck/fscheck.cpp — TEST-ONLY C entry points over csrc/host_fiat_shamir.h for a plain g++ build (no GPU, no library): the
// Fiat-Shamir codec with a SERIAL parallel-for, so that its pieces can be compared one by one with their Python twins
// (tests/test_fiat_shamir_host.py).
#include "host_fiat_shamir.h"

using namespace kzg_host;

static void serial_for(size_t n, const std::function<void(size_t)>& job) { for (size_t i = 0; i < n; ++i) job(i); }

extern "C" {
void fs_digest_to_fr_wire(const uint8_t dig[32], uint64_t out[4]) { digest_to_fr_wire(dig, out); }
void fs_fr_wire_to_be_bytes(const uint64_t wire[4], uint8_t out[32]) { fr_wire_to_be_bytes(wire, out); }
void fs_g1_serialize_compressed_ark(const uint64_t xy[8], uint8_t out[32]) { g1_serialize_compressed_ark(g1_from_wire(xy), out); }
size_t fs_blob_padded_len(size_t len) { return blob_padded_len(len); }
void fs_powers_of(const uint64_t r[4], size_t n, uint64_t* out) { powers_of(r, n, out); }
void fs_r_powers(const uint64_t* commitments, const uint64_t* zs, const uint64_t* ys, const uint64_t* proofs, const uint64_t* lens_elems, size_t n, uint64_t* out) {
    r_powers_host(commitments, zs, ys, proofs, lens_elems, n, out, serial_for);
}
void fs_multiproof_r_powers(const uint64_t* commitments, size_t n_commitments, const uint64_t* commitment_indices, const uint64_t* coset_indices, const uint64_t* ys,
                            const uint64_t* proofs, size_t count, size_t n, size_t l, uint64_t* out) {
    multiproof_r_powers_host(commitments, n_commitments, commitment_indices, coset_indices, ys, proofs, count, n, l, out, serial_for);
}
}
