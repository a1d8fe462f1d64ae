"""-m gpu: the encoder (`kzg_encode_cosets`, `KZG.encode_cosets`): the cosets of values and their proofs for d coefficients on a domain
of n = r d points, bit-equal to `kzg_compute_multiproofs` of the zero-padded coefficients, to known-tau values and to commitments of
the quotients, over an SRS of d points; every form of the padded transform (direct stages, radix-2 on lane pairs and on lanes, the
extreme spread), degenerate inputs, the protocol end to end (verify, recover), the error table, two threads and two contexts at once,
and the bound-checked build.  Bit-exact: np.array_equal on the wire limbs."""
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

import pyref
from pyref import R_

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G1 = (1, 2)
TAU = int.from_bytes(__import__("hashlib").sha256(b"kzg-bn254-mi355x/encode/v1").digest(), "big") % R_


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


@pytest.fixture(scope="module")
def ref_srs(k, test_srs_wire):
    return k.SRS(test_srs_wire, order=3000)


def rand_ints(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R_) for _ in range(n)]


def coeff_form(k, ints):
    return k.PolynomialCoeffForm(pyref.frs_to_mont(ints))


def div_xl(f, l, c):
    """f = q (X^l - c) + r: (q, r), coefficient lists"""
    f = list(f)
    q = [0] * (len(f) - l)
    for i in range(len(f) - 1, l - 1, -1):
        co = f[i]
        q[i - l] = co
        f[i] = 0
        f[i - l] = (f[i - l] + co * c) % R_
    return q, f[:l]


def wire_pt(v):
    return None if not np.asarray(v).any() else pyref.point_from_wire(v)


def raw_encode(k, srs, data, d, eval_form, n, l, values=True, proofs=True):
    ctx = srs.ctx
    L = k._lib
    data = np.ascontiguousarray(data, dtype=np.uint64).reshape(-1, 4)
    m = n // l
    ys = np.full((m, l, 4), 7, dtype=np.uint64)
    out = np.full((m, 8), 7, dtype=np.uint64)
    inf = np.full(m, 7, dtype=np.uint8)
    rc = L.load().kzg_encode_cosets(ctx.handle, srs.handle, L.ptr(data), d, eval_form, n, l, L.ptr(ys) if values else None,
                                    L.ptr(out) if proofs else None, inf.ctypes.data_as(L.u8p))
    assert rc == 0, (rc, ctx.last_error())
    return ys, out, inf


# ---- 1. equals the padded call: the direct form, on the reference's 3 000-point SRS ------------------------------------------------
SHAPES = [(2, 4, 1), (64, 128, 1), (256, 2048, 1), (256, 2048, 16), (1024, 2048, 512), (2048, 2048, 4)]
_padded = {}


def padded_reference(k, ref_srs, d, n, l):
    """(coeffs, evals of the padded coefficients, proofs of kzg_compute_multiproofs of them): computed once per shape"""
    key = (d, n, l)
    if key not in _padded:
        coeffs = rand_ints(d, 1000 * d + n + l)
        padded = coeffs + [0] * (n - d)
        proofs = k.KZG.new().compute_multiproofs(coeff_form(k, padded), ref_srs, l)
        proofs.setflags(write=False)
        _padded[key] = (coeffs, pyref.dft(padded), proofs)
    return _padded[key]


@pytest.mark.parametrize("d,n,l", SHAPES)
def test_equals_the_padded_call(k, ref_srs, d, n, l):
    coeffs, evals, want = padded_reference(k, ref_srs, d, n, l)
    m, r = n // l, n // d
    kzg = k.KZG.new()
    ys, proofs = kzg.encode_cosets(coeff_form(k, coeffs), ref_srs, n, l)
    assert ys.shape == (m, l, 4) and ys.dtype == np.uint64 and proofs.shape == (m, 8) and proofs.dtype == np.uint64
    assert np.array_equal(proofs, want)
    evals_wire = pyref.frs_to_mont(evals)
    assert np.array_equal(ys, kzg.cosets(k.PolynomialEvalForm(evals_wire), l))
    # eval form: the d evaluations on the d-point domain {(w^r)^i}
    evals_d = pyref.dft(coeffs)
    ys_e, proofs_e = kzg.encode_cosets(k.PolynomialEvalForm(pyref.frs_to_mont(evals_d)), ref_srs, n, l)
    assert np.array_equal(ys_e, ys) and np.array_equal(proofs_e, proofs)
    # evaluation index e = k + j m is ys[k][j]: the indices i r give the input evaluations back
    idx = np.arange(d) * r
    assert np.array_equal(ys[idx % m, idx // m], pyref.frs_to_mont(evals_d))


# ---- 2. an SRS of exactly d points ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", [1, 16])
def test_an_srs_of_d_points_suffices(k, ref_srs, test_srs_wire, l):
    d, n = 256, 2048
    coeffs, _, want = padded_reference(k, ref_srs, d, n, l)
    poly = coeff_form(k, coeffs)
    kzg = k.KZG.new()
    srs = k.SRS(test_srs_wire[:d], order=d)
    ys, proofs = kzg.encode_cosets(poly, srs, n, l)
    assert np.array_equal(proofs, want)
    # the padded call needs n points
    L = k._lib
    padded = np.ascontiguousarray(pyref.frs_to_mont(coeffs + [0] * (n - d)), dtype=np.uint64)
    out = np.zeros((n // l, 8), dtype=np.uint64)
    inf = np.zeros(n // l, dtype=np.uint8)
    assert L.load().kzg_compute_multiproofs(srs.ctx.handle, srs.handle, L.ptr(padded), n, 0, l, L.ptr(out), inf.ctypes.data_as(L.u8p)) == L.ERR_SRS_CAPACITY_EXCEEDED
    # the cache entry is the (d, l) one
    srs.drop_multiproof()
    srs.cache_multiproof(d, l)
    ys2, proofs2 = kzg.encode_cosets(poly, srs, n, l)
    assert np.array_equal(proofs2, want) and np.array_equal(ys2, ys)
    assert np.array_equal(kzg.compute_multiproofs(poly, srs, l), kzg.encode_cosets(poly, srs, d, l)[1])     # n = d: the same entry, the same proofs
    srs.drop_multiproof()
    ys3, proofs3 = kzg.encode_cosets(poly, srs, n, l)                  # rebuilt on use
    assert np.array_equal(proofs3, want) and np.array_equal(ys3, ys)
    srs.close()


# ---- 3. the radix-2 form on lane pairs: m = 2^15, known tau -------------------------------------------------------------------------
def check_sampled_against_the_closed_form(coeffs, n, ys, proofs, samples, seed):
    log_n = n.bit_length() - 1
    w = pyref.root_of_unity(log_n)
    f_tau = pyref.poly_eval(coeffs, TAU)
    for kk in random.Random(seed).sample(range(n), samples):
        c = pow(w, kk, R_)
        f_c = pyref.poly_eval(coeffs, c)
        s = (f_tau - f_c) * pow((TAU - c) % R_, -1, R_) % R_            # [(f(tau) - f(c)) / (tau - c)] G1
        assert wire_pt(proofs[kk]) == (None if s == 0 else pyref.ec_mul(s, G1)), kk
        assert np.array_equal(ys[kk, 0], pyref.fr_to_mont(f_c)), kk


def test_radix2_on_lane_pairs_equals_the_padded_call_and_the_closed_form(k):
    d, n = 1 << 12, 1 << 15
    coeffs = rand_ints(d, 31)
    kzg = k.KZG.new()
    srs_d = k.SRS.generate(TAU, d)
    ys, proofs = kzg.encode_cosets(coeff_form(k, coeffs), srs_d, n, 1)
    srs_d.close()
    srs_n = k.SRS.generate(TAU, n)
    want = kzg.compute_multiproofs(coeff_form(k, coeffs + [0] * (n - d)), srs_n, 1)
    srs_n.close()
    assert np.array_equal(proofs, want)                                 # all 2^15
    check_sampled_against_the_closed_form(coeffs, n, ys, proofs, 64, 32)


def test_radix2_on_lane_pairs_rate_half(k):
    d, n = 1 << 14, 1 << 15
    coeffs = rand_ints(d, 33)
    srs_d = k.SRS.generate(TAU, d)
    ys, proofs = k.KZG.new().encode_cosets(coeff_form(k, coeffs), srs_d, n, 1)
    srs_d.close()
    check_sampled_against_the_closed_form(coeffs, n, ys, proofs, 64, 34)


# ---- 4. the radix-2 form on lanes: m = 2^17 ---------------------------------------------------------------------------------------
def test_radix2_on_lanes(k):
    d, n = 1 << 14, 1 << 17
    coeffs = rand_ints(d, 41)
    srs_d = k.SRS.generate(TAU, d)
    ys, proofs = k.KZG.new().encode_cosets(coeff_form(k, coeffs), srs_d, n, 1)
    srs_d.close()
    check_sampled_against_the_closed_form(coeffs, n, ys, proofs, 32, 42)


# ---- 5. the extreme spread: two and four coefficients on 2^15 points -------------------------------------------------------------
def test_extreme_spread(k):
    n = 1 << 15
    kzg = k.KZG.new()
    a, b = rand_ints(2, 51)
    srs = k.SRS.generate(TAU, 2)
    ys, proofs = kzg.encode_cosets(coeff_form(k, [a, b]), srs, n, 1)
    srs.close()
    one = np.asarray(pyref.point_to_wire(pyref.ec_mul(b, G1)), dtype=np.uint64).reshape(8)     # (a + bX - f(z)) / (X - z) = b: [b] srs[0]
    assert np.array_equal(proofs, np.broadcast_to(one, (n, 8)))
    w = pyref.root_of_unity(15)
    for kk in random.Random(52).sample(range(n), 64):
        assert np.array_equal(ys[kk, 0], pyref.fr_to_mont((a + b * pow(w, kk, R_)) % R_)), kk
    coeffs = rand_ints(4, 53)
    srs = k.SRS.generate(TAU, 4)
    ys, proofs = kzg.encode_cosets(coeff_form(k, coeffs), srs, n, 1)
    srs.close()
    check_sampled_against_the_closed_form(coeffs, n, ys, proofs, 64, 54)


# ---- 6. degenerate inputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", [1, 4])
def test_zero_and_constant_polynomials_give_flagged_identities(k, ref_srs, l):
    d, n = 256, 1024
    for coeffs in ([0] * d, [12345] + [0] * (d - 1)):
        ys, out, inf = raw_encode(k, ref_srs, pyref.frs_to_mont(coeffs), d, 0, n, l)
        assert not out.any() and np.all(inf == 1)
        assert np.array_equal(ys, np.broadcast_to(np.asarray(pyref.fr_to_mont(coeffs[0]), dtype=np.uint64), (n // l, l, 4)))
    ys, out, inf = raw_encode(k, ref_srs, pyref.frs_to_mont([777] * d), d, 1, n, l)             # constant in eval form
    assert not out.any() and np.all(inf == 1)
    assert np.array_equal(ys, np.broadcast_to(np.asarray(pyref.fr_to_mont(777), dtype=np.uint64), (n // l, l, 4)))


def test_monomial_and_equal_coefficients(k, ref_srs):
    d, n, l = 512, 2048, 8
    m = n // l
    w = pyref.root_of_unity(11)
    kzg = k.KZG.new()
    for coeffs in ([0] * (d - 1) + [1], [5] * d):                      # X^(d-1); all-equal coefficients (equal points meet in the sums)
        ys, out, inf = raw_encode(k, ref_srs, pyref.frs_to_mont(coeffs), d, 0, n, l)
        assert np.array_equal(inf, (~out.any(axis=1)).astype(np.uint8))
        sample = [0, 1, m // 2, m - 1]
        quotients = [coeff_form(k, div_xl(coeffs, l, pow(w, kk * l, R_))[0]) for kk in sample]
        assert np.array_equal(out[sample], kzg.commit_coeff_form_batch(quotients, ref_srs))
        for kk in sample:
            assert np.array_equal(ys[kk, 3], pyref.fr_to_mont(pyref.poly_eval(coeffs, pow(w, kk + 3 * m, R_))))


def test_each_output_alone_is_identical(k, ref_srs):
    d, n, l = 256, 2048, 16
    coeffs, _, want = padded_reference(k, ref_srs, d, n, l)
    data = pyref.frs_to_mont(coeffs)
    ys, out, inf = raw_encode(k, ref_srs, data, d, 0, n, l)
    ys_v, out_v, inf_v = raw_encode(k, ref_srs, data, d, 0, n, l, proofs=False)
    assert np.array_equal(ys_v, ys) and np.all(out_v == 7) and np.all(inf_v == 7)               # nothing written for the output left out
    ys_p, out_p, inf_p = raw_encode(k, ref_srs, data, d, 0, n, l, values=False)
    assert np.array_equal(out_p, out) and np.array_equal(inf_p, inf) and np.all(ys_p == 7)
    assert np.array_equal(out, want)
    kzg = k.KZG.new()
    assert kzg.encode_cosets(coeff_form(k, coeffs), ref_srs, n, l, values=False)[0] is None
    assert kzg.encode_cosets(coeff_form(k, coeffs), ref_srs, n, l, proofs=False)[1] is None


# ---- 7. the protocol closes: encode, sample, verify, recover ----------------------------------------------------------------------
def test_the_protocol_closes(k):
    d, n, l = 512, 2048, 16
    m = n // l
    rnd = random.Random(71)
    coeffs = [rnd.randrange(R_) for _ in range(d)]
    poly = coeff_form(k, coeffs)
    srs = k.SRS.generate(TAU, d)
    kzg = k.KZG.new()
    commitment = kzg.commit_coeff_form(poly, srs)
    ys, proofs = kzg.encode_cosets(poly, srs, n, l)
    g2 = k.helpers.g2_mul_generator(k.fr.fr_from_int(pow(TAU, l, R_)))
    every = list(range(m))
    assert k.verifier.verify_multiproof_batch([commitment], [0] * m, every, ys, list(proofs), n, srs, g2) is True
    bad = ys.copy()
    bad[77, 5] = pyref.fr_to_mont(pyref.fr_from_mont(bad[77, 5]) + 1)  # one value changed
    assert k.verifier.verify_multiproof_batch([commitment], [0] * m, every, bad, list(proofs), n, srs, g2) is False
    ks = rnd.sample(range(m), 32)                                       # 32 cosets of 16 values: exactly d
    got = kzg.recover_from_cosets(ks, np.ascontiguousarray(ys[ks]), n, degree_bound=d, eval_form=False)
    assert np.array_equal(got.coeffs(), pyref.frs_to_mont(coeffs + [0] * (n - d)))
    srs.close()


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------
def test_error_table_then_a_bit_exact_proof(k, ref_srs, test_srs_wire):
    L = k._lib
    lib = L.load()
    ctx = ref_srs.ctx
    kzg = k.KZG.new()
    kzg.calculate_and_store_roots_of_unity(64 * 32)
    evals = k.PolynomialEvalForm(pyref.frs_to_mont(rand_ints(64, 81)))
    z = kzg.get_roots_of_unities()[3]
    before = kzg.compute_proof(evals, z, ref_srs)
    big = np.zeros((1 << 12, 4), dtype=np.uint64)
    ys = np.full((1 << 12, 4), 7, dtype=np.uint64)
    out = np.full((1 << 12, 8), 7, dtype=np.uint64)
    inf = np.full(1 << 12, 7, dtype=np.uint8)
    lag = ref_srs.lagrange(64)
    other_ctx = L.Context(0)
    other_srs = k.SRS(test_srs_wire[:64], order=64, ctx=other_ctx)
    NOARG = object()

    def call(srs_h, d, n, l, data=big, ctx_h=ctx.handle, ys_p=NOARG, out_p=NOARG, inf_p=NOARG):
        return lib.kzg_encode_cosets(ctx_h, srs_h, None if data is None else L.ptr(data), d, 0, n, l, L.ptr(ys) if ys_p is NOARG else ys_p,
                                     L.ptr(out) if out_p is NOARG else out_p, inf.ctypes.data_as(L.u8p) if inf_p is NOARG else inf_p)

    h = ref_srs.handle
    # 1. null pointers, no output, proofs without flags -- in front of a length that is no power of two
    assert call(h, 3, 0, 1, ctx_h=None) == L.ERR_INVALID_ARG
    assert call(None, 3, 0, 1) == L.ERR_INVALID_ARG
    assert call(h, 3, 0, 1, data=None) == L.ERR_INVALID_ARG
    assert call(h, 3, 0, 1, ys_p=None, out_p=None) == L.ERR_INVALID_ARG
    assert call(h, 3, 0, 1, inf_p=None) == L.ERR_INVALID_ARG
    # 2. an SRS of another context, a Lagrange-basis handle -- in front of the same
    assert call(other_srs.handle, 3, 0, 1) == L.ERR_INVALID_ARG
    assert call(lag.handle, 3, 0, 1) == L.ERR_INVALID_ARG
    # 3. lengths -- in front of the domain limit
    assert call(h, 0, 64, 1) == L.ERR_NOT_POWER_OF_TWO
    assert call(h, 48, 1 << 25, 1) == L.ERR_NOT_POWER_OF_TWO
    assert call(h, 64, 0, 1) == L.ERR_NOT_POWER_OF_TWO
    assert call(h, 64, 96, 1) == L.ERR_NOT_POWER_OF_TWO
    # 4. the domain limit -- in front of the shape rules
    assert call(h, 1, 1 << 25, 3) == L.ERR_DOMAIN
    # 5. shapes -- in front of the SRS capacity
    assert call(h, 4096, 2048, 1) == L.ERR_INVALID_ARG                  # poly_len > n
    assert call(h, 1, 64, 1) == L.ERR_INVALID_ARG                       # poly_len = 1
    assert call(h, 4096, 4096, 0) == L.ERR_INVALID_ARG
    assert call(h, 4096, 4096, 3) == L.ERR_INVALID_ARG                  # l not a power of two
    assert call(h, 64, 4096, 64) == L.ERR_INVALID_ARG                   # l > poly_len / 2 though l <= n / 2
    # 6. the SRS holds 3 000 points
    assert call(h, 4096, 4096, 1) == L.ERR_SRS_CAPACITY_EXCEEDED
    assert call(other_srs.handle, 128, 256, 1, ctx_h=other_ctx.handle) == L.ERR_SRS_CAPACITY_EXCEEDED
    assert np.all(ys == 7) and np.all(out == 7) and np.all(inf == 7)    # no output touched
    # flags are not needed for values alone
    assert call(h, 64, 128, 1, out_p=None, inf_p=None) == 0
    assert np.all(out == 7) and np.all(inf == 7) and not np.all(ys[:128] == 7) and np.all(ys[128:] == 7)
    # the context still computes the same proof
    assert np.array_equal(kzg.compute_proof(evals, z, ref_srs), before)
    # the Python surface
    poly = coeff_form(k, rand_ints(64, 82))
    with pytest.raises(k.errors.GenericError):
        kzg.encode_cosets(poly, ref_srs, 256, 3)
    with pytest.raises(k.errors.GenericError):
        kzg.encode_cosets(poly, ref_srs, 256, 64)
    with pytest.raises(k.errors.FFTError):
        kzg.encode_cosets(poly, ref_srs, 96, 1)
    with pytest.raises(k.errors.SrsCapacityExceeded):
        kzg.encode_cosets(k.PolynomialCoeffForm(big), ref_srs, 4096, 1)
    with pytest.raises(ValueError):                                     # KZG_ERR_INVALID_ARG, as everywhere in the library
        kzg.encode_cosets(poly, lag, 256, 1)
    assert np.array_equal(kzg.compute_proof(evals, z, ref_srs), before)
    lag.close()
    other_srs.close()
    other_ctx.close()


# ---- 9. two threads on one context, a second context beside them -----------------------------------------------------------------
def test_threads_and_contexts_at_once(k, test_srs_wire):
    d, n, l = 512, 2048, 4
    coeffs = rand_ints(d, 91)
    poly = coeff_form(k, coeffs)
    ctx_a = k._lib.Context(0)
    ctx_b = k._lib.Context(0)
    srs_a = k.SRS(test_srs_wire[:d], order=d, ctx=ctx_a)
    srs_b = k.SRS(test_srs_wire[:d], order=d, ctx=ctx_b)
    kz_a, kz_b = k.KZG.new(ctx_a), k.KZG.new(ctx_b)
    # expected values, one call at a time, before anything runs concurrently
    one = k.SRS(test_srs_wire[:d], order=d)
    kz = k.KZG.new()
    want_ys, want_proofs = kz.encode_cosets(poly, one, n, l)
    want_mp = kz.compute_multiproofs(poly, one, l)
    want_ys8, want_proofs8 = kz.encode_cosets(poly, one, 4 * n, l)
    one.close()
    errors, results = [], {}

    def run(name, fn):
        try:
            results[name] = fn()
        except Exception as e:                                          # reported below
            errors.append((name, repr(e)))

    def encode():                                                       # whichever of the two comes first builds the (d, l) entry on srs_a
        return [kz_a.encode_cosets(poly, srs_a, n, l) for _ in range(3)]

    def multi():
        return [kz_a.compute_multiproofs(poly, srs_a, l) for _ in range(3)]

    def other():
        return [kz_b.encode_cosets(poly, srs_b, 4 * n, l) for _ in range(3)]

    ts = [threading.Thread(target=run, args=(nm, fn)) for nm, fn in (("encode", encode), ("multi", multi), ("other", other))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert all(np.array_equal(y, want_ys) and np.array_equal(p, want_proofs) for y, p in results["encode"])
    assert all(np.array_equal(r, want_mp) for r in results["multi"])
    assert all(np.array_equal(y, want_ys8) and np.array_equal(p, want_proofs8) for y, p in results["other"])
    srs_a.close(); srs_b.close()
    ctx_a.close(); ctx_b.close()


# ---- 10. the bound-checked build runs tests 1-6 with every site counter at 0 ------------------------------------------------------
VARIANT = os.path.join(ROOT, "rust-kzg-bn254_amd", "libkzg_bn254_mi355x_boundcheck.so")
CHILD = r'''
import ctypes as C, os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import torch  # noqa: F401  (load order: tests/conftest.py)
import rust_kzg_bn254_amd  # noqa: F401
L = [m for name, m in list(sys.modules.items()) if name.endswith("_lib") and hasattr(m, "LIB_PATH")][0]
assert L.LIB_PATH == os.environ["KZG_LIB_PATH"], L.LIB_PATH
h = L.load()
n = h.kzg_bc_sites()
assert h.kzg_bc_reset_all() == 0
import pytest
rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", "-x", *%(tests)r])
counts = (C.c_ulonglong * n)()
first = (C.c_int32 * (9 * n))()
assert h.kzg_bc_read_all(counts, first) == 0
print("PYTEST_RC", int(rc))
for s in range(n):
    print("SITE", s, counts[s])
'''
WORKLOAD = ["tests/test_gpu_encode.py::" + t for t in (
    "test_equals_the_padded_call", "test_an_srs_of_d_points_suffices", "test_radix2_on_lane_pairs_equals_the_padded_call_and_the_closed_form",
    "test_radix2_on_lane_pairs_rate_half", "test_radix2_on_lanes", "test_extreme_spread", "test_zero_and_constant_polynomials_give_flagged_identities",
    "test_monomial_and_equal_coefficients", "test_each_output_alone_is_identical")]


def test_bound_checked_build_keeps_every_precondition():
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": WORKLOAD}], capture_output=True, text=True, timeout=1500,
                         env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "PYTEST_RC 0" in out, (out[-3000:], res.stderr[-2000:])
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert sites
    fired = {int(s[1]): int(s[2]) for s in sites if int(s[2])}
    assert not fired, fired
