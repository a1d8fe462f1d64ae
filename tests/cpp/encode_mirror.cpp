// tests/cpp/encode_mirror.cpp -- KZG::encode_cosets of the C++ mirror (include/kzg_bn254_mi355x.hpp) as its own process: encodes
// f_i = (i + 3)^2, i < 64, on 256 points in cosets of 4 over SRS::generate(tau, 64) -- an SRS of exactly d points -- from coefficient
// form and from evaluation form, prints the values and the proofs as hex for tests/test_gpu_encode_cpp_mirror.py to compare with the
// Python mirror, and checks the errors the method raises before it calls the library.  usage: encode_mirror <tau: 64 hex digits>
#include <cstdio>
#include <string>
#include <vector>

#include "kzg_bn254_mi355x.hpp"

using namespace rust_kzg_bn254;

static std::string hex(const uint64_t* w, size_t n) {
    std::string s;
    char buf[17];
    for (size_t i = 0; i < n; ++i) { std::snprintf(buf, sizeof buf, "%016llx", (unsigned long long)w[i]); s += buf; }
    return s;
}
template <class F> static bool raises(KzgError::Kind kind, F f) {
    try { f(); } catch (const KzgError& e) { return e.kind == kind; }
    return false;
}
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "encode_mirror: line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <tau: 64 hex digits>\n", argv[0]); return 2; }
    uint8_t tau_be[32];
    for (int i = 0; i < 32; ++i) { unsigned v = 0; std::sscanf(argv[1] + 2 * i, "%2x", &v); tau_be[i] = (uint8_t)v; }
    const size_t d = 64, n = 256, l = 4, m = n / l;
    try {
        const SRS srs = SRS::generate(Fr::from_be_bytes_mod_order(tau_be), d);
        std::vector<Fr> coeffs(d);
        for (size_t i = 0; i < d; ++i) coeffs[i] = Fr::from_u64((i + 3) * (i + 3));
        const PolynomialCoeffForm poly = PolynomialCoeffForm::new_(coeffs);
        const KZG prover = KZG::new_();
        const KZG::EncodedCosets enc = prover.encode_cosets(poly, srs, n, l);
        CHECK(enc.ys.size() == n && enc.proofs.size() == m);
        // eval form: the evaluations on the d-point domain are ys at the evaluation indices i r, index e = k + j m being ys[k l + j]
        std::vector<Fr> evals(d);
        for (size_t i = 0; i < d; ++i) { const size_t e = i * (n / d); evals[i] = enc.ys[(e % m) * l + e / m]; }
        const KZG::EncodedCosets again = prover.encode_cosets(PolynomialEvalForm::new_(evals), srs, n, l);
        CHECK(again.ys == enc.ys && again.proofs == enc.proofs);
        const KZG::EncodedCosets only_values = prover.encode_cosets(poly, srs, n, l, true, false), only_proofs = prover.encode_cosets(poly, srs, n, l, false, true);
        CHECK(only_values.ys == enc.ys && only_values.proofs.empty() && only_proofs.proofs == enc.proofs && only_proofs.ys.empty());
        CHECK(raises(KzgError::Kind::GenericError, [&] { prover.encode_cosets(poly, srs, n, 3); }));
        CHECK(raises(KzgError::Kind::GenericError, [&] { prover.encode_cosets(poly, srs, n, 64); }));
        CHECK(raises(KzgError::Kind::GenericError, [&] { prover.encode_cosets(poly, srs, 32, 1); }));
        CHECK(raises(KzgError::Kind::GenericError, [&] { prover.encode_cosets(poly, srs, n, l, false, false); }));
        CHECK(raises(KzgError::Kind::FFTError, [&] { prover.encode_cosets(poly, srs, 96, 1); }));
        std::vector<Fr> longer(128, Fr::one());
        CHECK(raises(KzgError::Kind::SrsCapacityExceeded, [&] { prover.encode_cosets(PolynomialCoeffForm::new_(longer), srs, n, l); }));
        std::printf("ys %s\n", hex(enc.ys.data()->limbs.data(), 4 * n).c_str());
        std::printf("proofs %s\n", hex(enc.proofs.data()->xy.data(), 8 * m).c_str());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "encode_mirror: %s\n", e.what());
        return 1;
    }
    std::printf("encode_mirror ok\n");
    return 0;
}
