"""-m gpu: the blob header in one call (`kzg_commit_with_length_proof`) and its verification.  Setup of order N = 2^16 with a known tau, a
trailing G2 handle generated at first_power = 2^16 - 2^12, claimed lengths 2^10 and 2^12, polynomials shorter than and as long as the
claim: the three outputs equal the three separate calls bit for bit and the closed forms [f(tau)]_1, [f(tau)]_2, [tau^(N-d) f(tau)]_2; the
verifier accepts, rejects every altered element and rejects an honest 2^12-coefficient header presented as length 2^11; the errors come in
the documented order; and the encoder's promise closes the loop (encode with d = claimed_len, recover with that degree bound)."""
import ctypes as C
import random

import numpy as np
import pytest

import rust_kzg_bn254_amd as k
from pyref import R_
from rust_kzg_bn254_amd import _lib, helpers, verifier
from rust_kzg_bn254_amd.errors import FFTError, SerializationError, SrsCapacityExceeded
from rust_kzg_bn254_amd.fr import fr_from_int, frs_from_ints

pytestmark = pytest.mark.gpu
TAU = 0x2B992DDFA23249D6A1B5C4D3E2F10987
N = 1 << 16
TRAIL = 1 << 12


def horner(coeffs):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * TAU + c) % R_
    return acc


@pytest.fixture(scope="module")
def setup():
    g1 = k.SRS.generate(TAU, TRAIL)                                  # the monomial powers the polynomials need
    g2 = k.G2SRS.generate(TAU, TRAIL)
    trailing = k.G2SRS.generate(TAU, TRAIL, first_power=N - TRAIL)
    yield g1, g2, trailing
    for h in (g1, g2, trailing):
        h.close()


def shift_g1(d):
    s = k.SRS.generate(TAU, 1, first_power=N - d)
    try:
        return s.g1[0].copy()
    finally:
        s.close()


@pytest.mark.parametrize("d,n", [(1 << 10, 1 << 9), (1 << 10, 1 << 10), (1 << 12, 1 << 10), (1 << 12, 1 << 12)])
def test_header_equals_the_separate_calls_and_the_closed_forms(setup, d, n):
    g1, g2, trailing = setup
    rnd = random.Random(d + n)
    coeffs = [rnd.randrange(R_) for _ in range(n)]
    poly = k.PolynomialCoeffForm(frs_from_ints(coeffs))
    kzg = k.KZG.new()
    c, c2, pi2 = kzg.commit_with_length_proof(poly, g1, g2, trailing, N, d)
    ft = horner(coeffs)
    assert np.array_equal(c, kzg.commit_coeff_form(poly, g1))
    assert np.array_equal(c2, kzg.commit_g2_coeff_form(poly, g2))
    ctx = _lib.default_context()
    sep = np.zeros(16, np.uint64); inf = C.c_uint8(0)
    sc = np.ascontiguousarray(poly.coeffs())
    assert _lib.load().kzg_msm_g2_srs(ctx.handle, trailing.handle, TRAIL - d, _lib.ptr(sc), n, _lib.ptr(sep), C.byref(inf)) == _lib.OK
    assert np.array_equal(pi2, sep)
    assert np.array_equal(c2, helpers.g2_mul_generator(fr_from_int(ft)))
    assert np.array_equal(pi2, helpers.g2_mul_generator(fr_from_int(ft * pow(TAU, N - d, R_) % R_)))
    shift = shift_g1(d)
    assert verifier.verify_length_proof(c, c2, pi2, shift)
    other1 = g1.g1[5]
    other2 = helpers.g2_mul_generator(fr_from_int(12345))
    assert not verifier.verify_length_proof(other1, c2, pi2, shift)
    assert not verifier.verify_length_proof(c, other2, pi2, shift)
    assert not verifier.verify_length_proof(c, c2, other2, shift)
    assert not verifier.verify_length_proof(c, c2, pi2, shift_g1(d // 2))


def test_a_polynomial_of_4096_coefficients_cannot_claim_2048(setup):
    g1, g2, trailing = setup
    rnd = random.Random(1)
    coeffs = [rnd.randrange(R_) for _ in range(1 << 12)]
    poly = k.PolynomialCoeffForm(frs_from_ints(coeffs))
    c, c2, pi2 = k.KZG.new().commit_with_length_proof(poly, g1, g2, trailing, N, 1 << 12)
    assert verifier.verify_length_proof(c, c2, pi2, shift_g1(1 << 12))
    assert not verifier.verify_length_proof(c, c2, pi2, shift_g1(1 << 11))       # presented with claimed_len 2^11
    with pytest.raises(ValueError):                                               # and the prover's call refuses n > claimed_len
        k.KZG.new().commit_with_length_proof(poly, g1, g2, trailing, N, 1 << 11)


def test_errors_in_the_documented_order(setup):
    g1, g2, trailing = setup
    ctx = _lib.default_context()
    lib = _lib.load()
    sc = np.ascontiguousarray(frs_from_ints(list(range(1, 9))))
    c = np.zeros(8, np.uint64); c2 = np.zeros(16, np.uint64); pi2 = np.zeros(16, np.uint64)

    def call(g1h=g1.handle, g2h=g2.handle, trh=trailing.handle, first=N - TRAIL, order=N, n=8, d=8, scalars=sc, out=c):
        return lib.kzg_commit_with_length_proof(ctx.handle, g1h, g2h, trh, first, order, None if scalars is None else _lib.ptr(scalars), n, d,
                                                None if out is None else _lib.ptr(out), _lib.ptr(c2), _lib.ptr(pi2))
    assert call() == _lib.OK
    # 1. null pointers win over everything else
    assert call(g1h=None, order=3) == _lib.ERR_INVALID_ARG
    assert call(trh=None, d=3) == _lib.ERR_INVALID_ARG
    assert call(scalars=None, order=3) == _lib.ERR_INVALID_ARG
    assert call(out=None, d=5) == _lib.ERR_INVALID_ARG
    # 2. powers of two, before the size relations
    assert call(order=N - 1, n=9, d=8) == _lib.ERR_NOT_POWER_OF_TWO
    assert call(d=12, n=13) == _lib.ERR_NOT_POWER_OF_TWO
    assert call(d=0, n=0) == _lib.ERR_NOT_POWER_OF_TWO
    # 3. n > claimed_len, claimed_len > srs_order -- before the window check (first_power beyond the order would fail that one)
    assert call(n=8, d=4, first=N) == _lib.ERR_INVALID_ARG
    assert call(order=4, d=8, first=N) == _lib.ERR_INVALID_ARG
    # 4. the window [N - d, N) inside the trailing handle -- before the length check (n = 8 > a 4-point SRS would fail that one)
    tiny1 = k.SRS.generate(TAU, 4); tiny2 = k.G2SRS.generate(TAU, 4)
    try:
        assert call(d=2 * TRAIL, g1h=tiny1.handle) == _lib.ERR_SRS_CAPACITY_EXCEEDED          # starts before the handle's first power
        assert call(first=N - 2 * TRAIL, g1h=tiny1.handle) == _lib.ERR_SRS_CAPACITY_EXCEEDED  # ends behind its last point
        assert call(order=2 * N, g2h=tiny2.handle) == _lib.ERR_SRS_CAPACITY_EXCEEDED
        # 5. n larger than either monomial SRS
        assert call(g1h=tiny1.handle) == _lib.ERR_POLY_LENGTH
        assert call(g2h=tiny2.handle) == _lib.ERR_POLY_LENGTH
        assert call(g1h=tiny1.handle, g2h=tiny2.handle, n=4) == _lib.OK
    finally:
        tiny1.close(); tiny2.close()
    # the Python surface maps them as its neighbours do
    kzg = k.KZG.new()
    poly = k.PolynomialCoeffForm(sc)
    with pytest.raises(FFTError):
        kzg.commit_with_length_proof(poly, g1, g2, trailing, N, 12)
    with pytest.raises(SrsCapacityExceeded):
        kzg.commit_with_length_proof(poly, g1, g2, trailing, N, 2 * TRAIL)
    # n = 0: three identities
    assert call(n=0, scalars=None) == _lib.OK and not c.any() and not c2.any() and not pi2.any()
    # the context is usable after all of that
    assert call() == _lib.OK and c.any()


def test_the_encoders_promise_closes_the_loop(setup):
    """deg f < d is what `encode_cosets` relies on (d SRS points, a (d, l) table, a shortened FFT) and what `recover_from_cosets` reports:
    here the header that proves it verifies, and the polynomial recovered under that bound is the one committed to."""
    g1, g2, trailing = setup
    d, rate, l = 1 << 10, 4, 16
    n = rate * d
    rnd = random.Random(3)
    coeffs = [rnd.randrange(R_) for _ in range(d)]
    poly = k.PolynomialCoeffForm(frs_from_ints(coeffs))
    kzg = k.KZG.new()
    c, c2, pi2 = kzg.commit_with_length_proof(poly, g1, g2, trailing, N, d)
    assert verifier.verify_length_proof(c, c2, pi2, shift_g1(d))
    ys, _ = kzg.encode_cosets(poly, g1, n, l, proofs=False)
    ks = rnd.sample(range(n // l), d // l)
    got = kzg.recover_from_cosets(ks, np.ascontiguousarray(ys[ks]), n, degree_bound=d, eval_form=False)
    assert np.array_equal(got.coeffs()[:d], poly.coeffs()) and not got.coeffs()[d:].any()
    assert np.array_equal(kzg.commit_coeff_form(k.PolynomialCoeffForm(got.coeffs()[:d]), g1), c)
