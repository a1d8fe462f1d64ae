"""-m gpu: the FK20 multi-proofs (`kzg_compute_multiproofs`, `KZG.compute_multiproofs`): every coset proof of a domain in one call,
bit-equal to the one-point proofs, to commitments of the quotients and to known-tau values; the SRS cache, the error table, two
threads and two contexts at once, and the bound-checked build.  Bit-exact: np.array_equal on the wire limbs."""
import ctypes as C
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
TAU = int.from_bytes(__import__("hashlib").sha256(b"kzg-bn254-mi355x/multiproof/v1").digest(), "big") % R_


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


def kzg_for(k, n):
    kzg = k.KZG.new()
    kzg.calculate_and_store_roots_of_unity(n * 32)
    assert len(kzg.get_roots_of_unities()) == n
    return kzg


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


# ---- 1. l = 1 on the reference's 3 000-point SRS: the proofs of compute_proof_with_known_z_fr_index ------------------------------
@pytest.mark.parametrize("n", [2, 4, 64, 1024, 2048])
def test_l1_equals_compute_proof_at_every_domain_point(k, ref_srs, n):
    evals = rand_ints(n, 100 + n)
    poly = k.PolynomialEvalForm(pyref.frs_to_mont(evals))
    kzg = kzg_for(k, n)
    got = kzg.compute_multiproofs(poly, ref_srs, 1)
    assert got.shape == (n, 8) and got.dtype == np.uint64
    roots = kzg.get_roots_of_unities()
    want = np.array(list(kzg.compute_proof_stream(((poly, roots[i]) for i in range(n)), ref_srs)))
    assert np.array_equal(got, want)
    if n == 2048:                                                  # a pairing check of every proof needs the SRS's [tau]G2: a known-tau SRS
        srs = k.SRS.generate(TAU, n)
        got = kzg.compute_multiproofs(poly, srs, 1)
        commitment = kzg.commit_eval_form(poly, srs)
        g2_tau = k.helpers.g2_mul_generator(k.fr.fr_from_int(TAU))
        ev = pyref.frs_to_mont(evals)
        for i in range(n):
            assert k.verifier.verify_proof(commitment, got[i], ev[i], roots[i], g2_tau), i
        assert not k.verifier.verify_proof(commitment, got[1], ev[0], roots[0], g2_tau)
        srs.close()


# ---- 2. l > 1: commitments of the quotients by X^l - w^(k l) --------------------------------------------------------------------
@pytest.mark.parametrize("l", [2, 16, 256, 1024])
def test_cosets_equal_commitments_of_the_quotients(k, ref_srs, l):
    n = 2048
    m = n // l
    coeffs = rand_ints(n, 200 + l)
    poly = k.PolynomialCoeffForm(pyref.frs_to_mont(coeffs))
    got = kzg_for(k, n).compute_multiproofs(poly, ref_srs, l)
    assert got.shape == (m, 8)
    w = pyref.root_of_unity(11)
    quotients = [k.PolynomialCoeffForm(pyref.frs_to_mont(div_xl(coeffs, l, pow(w, kk * l, R_))[0])) for kk in range(m)]
    want = np.concatenate([k.KZG.new().commit_coeff_form_batch(quotients[s:s + 64], ref_srs) for s in range(0, m, 64)])
    assert np.array_equal(got, want)


# ---- 3. known tau at 2^16 --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tau_srs(k):
    return k.SRS.generate(TAU, 1 << 16)


@pytest.mark.parametrize("l", [1, 64])
def test_known_tau_values_and_one_pairing(k, tau_srs, l):
    n = 1 << 16
    m = n // l
    coeffs = rand_ints(n, 300 + l)
    poly = k.PolynomialCoeffForm(pyref.frs_to_mont(coeffs))
    got = kzg_for(k, n).compute_multiproofs(poly, tau_srs, l)
    assert got.shape == (m, 8)
    w = pyref.root_of_unity(16)
    f_tau = pyref.poly_eval(coeffs, TAU)
    tau_l = pow(TAU, l, R_)
    ks = random.Random(l).sample(range(m), 64)
    for kk in ks:
        c = pow(w, kk * l, R_)
        # r_k = f mod (X^l - c): r_i = sum_j f_{i + j l} c^j
        r = [pyref.poly_eval(coeffs[i::l], c) for i in range(l)]
        r_tau = pyref.poly_eval(r, TAU)
        want = pyref.ec_mul((f_tau - r_tau) * pow((tau_l - c) % R_, -1, R_), G1)
        assert wire_pt(got[kk]) == want, kk
    if l == 64:
        kk = ks[0]
        c = pow(w, kk * l, R_)
        r_tau = pyref.poly_eval([pyref.poly_eval(coeffs[i::l], c) for i in range(l)], TAU)
        commitment = k.KZG.new().commit_coeff_form(poly, tau_srs)
        lhs_g2 = k.helpers.g2_mul_generator(pyref.fr_to_mont((tau_l - c) % R_))
        b1 = pyref.ec_add(pyref.point_from_wire(commitment), pyref.ec_neg(pyref.ec_mul(r_tau, G1)))
        assert k.helpers.pairings_verify(got[kk], lhs_g2, pyref.point_to_wire(b1), k.helpers.g2_generator())
        assert not k.helpers.pairings_verify(got[ks[1]], lhs_g2, pyref.point_to_wire(b1), k.helpers.g2_generator())


# ---- 4. degenerate inputs --------------------------------------------------------------------------------------------------------
def raw_multiproofs(k, srs, data, n, eval_form, l):
    ctx = srs.ctx
    data = np.ascontiguousarray(data, dtype=np.uint64).reshape(-1, 4)
    out = np.full((n // l, 8), 7, dtype=np.uint64)
    inf = np.full(n // l, 7, dtype=np.uint8)
    rc = k._lib.load().kzg_compute_multiproofs(ctx.handle, srs.handle, k._lib.ptr(data), n, eval_form, l, k._lib.ptr(out),
                                               inf.ctypes.data_as(k._lib.u8p))
    assert rc == 0, (rc, ctx.last_error())
    return out, inf


@pytest.mark.parametrize("l", [1, 4])
def test_zero_and_constant_polynomials_give_flagged_identities(k, ref_srs, l):
    n = 256
    for coeffs in ([0] * n, [12345] + [0] * (n - 1)):
        out, inf = raw_multiproofs(k, ref_srs, pyref.frs_to_mont(coeffs), n, 0, l)
        assert not out.any() and np.all(inf == 1)
    out, inf = raw_multiproofs(k, ref_srs, pyref.frs_to_mont([777] * n), n, 1, l)     # constant in eval form
    assert not out.any() and np.all(inf == 1)


@pytest.mark.parametrize("l", [1, 8])
def test_monomial_and_equal_coefficients(k, ref_srs, l):
    n = 512
    m = n // l
    w = pyref.root_of_unity(9)
    kzg = kzg_for(k, n)
    for coeffs in ([0] * (n - 1) + [1], [5] * n):                  # X^(n-1); all-equal coefficients (equal points meet in the sums)
        out, inf = raw_multiproofs(k, ref_srs, pyref.frs_to_mont(coeffs), n, 0, l)
        assert np.array_equal(inf, (~out.any(axis=1)).astype(np.uint8))
        sample = [0, 1, m // 2, m - 1]
        quotients = [k.PolynomialCoeffForm(pyref.frs_to_mont(div_xl(coeffs, l, pow(w, kk * l, R_))[0])) for kk in sample]
        want = kzg.commit_coeff_form_batch(quotients, ref_srs)
        assert np.array_equal(out[sample], want)


def test_eval_form_and_coeff_form_agree(k, ref_srs):
    n = 1024
    coeffs = rand_ints(n, 401)
    evals = pyref.dft(coeffs)
    kzg = kzg_for(k, n)
    for l in (1, 32):
        a = kzg.compute_multiproofs(k.PolynomialCoeffForm(pyref.frs_to_mont(coeffs)), ref_srs, l)
        b = kzg.compute_multiproofs(k.PolynomialEvalForm(pyref.frs_to_mont(evals)), ref_srs, l)
        assert np.array_equal(a, b)


# ---- 5. the cache ----------------------------------------------------------------------------------------------------------------
def test_cache_lazy_explicit_drop_rebuild_and_free(k, test_srs_wire):
    n = 512
    poly = k.PolynomialCoeffForm(pyref.frs_to_mont(rand_ints(n, 501)))
    kzg = k.KZG.new()
    srs = k.SRS(test_srs_wire[:1024], order=1024)
    lazy = kzg.compute_multiproofs(poly, srs, 1)                   # builds (512, 1) on first use
    lazy4 = kzg.compute_multiproofs(poly, srs, 4)                  # a second (n, l) beside it
    assert np.array_equal(kzg.compute_multiproofs(poly, srs, 1), lazy)
    srs.drop_multiproof()
    srs.cache_multiproof(n, 4)                                      # explicit
    srs.cache_multiproof(n, 1)
    srs.cache_multiproof(n, 1)                                      # already there: no-op
    assert np.array_equal(kzg.compute_multiproofs(poly, srs, 4), lazy4)
    assert np.array_equal(kzg.compute_multiproofs(poly, srs, 1), lazy)
    srs.drop_multiproof()
    srs.drop_multiproof()                                           # twice: nothing left to drop
    assert np.array_equal(kzg.compute_multiproofs(poly, srs, 1), lazy)   # rebuilt
    other = k.SRS(test_srs_wire[:1024], order=1024)                 # same points, a cache of its own
    assert np.array_equal(kzg.compute_multiproofs(poly, other, 4), lazy4)
    srs.close()                                                     # kzg_srs_free with two caches attached
    other.close()


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------
def test_error_table_then_a_bit_exact_proof(k, ref_srs, test_srs_wire):
    L = k._lib
    lib = L.load()
    ctx = ref_srs.ctx
    n = 64
    evals = pyref.frs_to_mont(rand_ints(n, 601))
    poly = k.PolynomialEvalForm(evals)
    kzg = kzg_for(k, n)
    z = kzg.get_roots_of_unities()[3]
    before = kzg.compute_proof(poly, z, ref_srs)
    big = np.zeros((1 << 12, 4), dtype=np.uint64)
    out = np.zeros((1 << 12, 8), dtype=np.uint64)
    inf = np.zeros(1 << 12, dtype=np.uint8)
    lag = ref_srs.lagrange(64)
    other_ctx = L.Context(0)
    other_srs = k.SRS(test_srs_wire[:64], order=64, ctx=other_ctx)

    def call(srs_h, data, nn, l, ctx_h=ctx.handle, out_p=L.ptr(out), inf_p=inf.ctypes.data_as(L.u8p)):
        return lib.kzg_compute_multiproofs(ctx_h, srs_h, None if data is None else L.ptr(data), nn, 1, l, out_p, inf_p)

    assert call(ref_srs.handle, None, n, 1) == L.ERR_INVALID_ARG
    assert call(ref_srs.handle, big, n, 1, out_p=None) == L.ERR_INVALID_ARG
    assert call(ref_srs.handle, big, n, 1, inf_p=None) == L.ERR_INVALID_ARG
    assert call(None, big, n, 1) == L.ERR_INVALID_ARG
    assert call(ref_srs.handle, big, n, 1, ctx_h=None) == L.ERR_INVALID_ARG
    assert call(other_srs.handle, big, 64, 1) == L.ERR_INVALID_ARG                  # srs->ctx != ctx
    assert call(lag.handle, big, 64, 1) == L.ERR_INVALID_ARG                        # Lagrange-basis handle
    assert call(ref_srs.handle, big, 1, 1) == L.ERR_INVALID_ARG                     # n = 1
    assert call(ref_srs.handle, big, 64, 3) == L.ERR_INVALID_ARG                    # l not a power of two
    assert call(ref_srs.handle, big, 64, 0) == L.ERR_INVALID_ARG
    assert call(ref_srs.handle, big, 64, 64) == L.ERR_INVALID_ARG                   # l > n / 2
    assert call(ref_srs.handle, big, 0, 1) == L.ERR_NOT_POWER_OF_TWO
    assert call(ref_srs.handle, big, 96, 1) == L.ERR_NOT_POWER_OF_TWO
    assert call(ref_srs.handle, big, 1 << 25, 1) == L.ERR_DOMAIN
    assert call(ref_srs.handle, big, 4096, 1) == L.ERR_SRS_CAPACITY_EXCEEDED
    assert lib.kzg_srs_cache_multiproof(ctx.handle, ref_srs.handle, 4096, 1) == L.ERR_SRS_CAPACITY_EXCEEDED
    assert lib.kzg_srs_cache_multiproof(ctx.handle, ref_srs.handle, 64, 33) == L.ERR_INVALID_ARG
    assert lib.kzg_srs_cache_multiproof(ctx.handle, lag.handle, 64, 1) == L.ERR_INVALID_ARG
    assert lib.kzg_srs_drop_multiproof(ctx.handle, other_srs.handle) == L.ERR_INVALID_ARG
    assert lib.kzg_srs_drop_multiproof(None, ref_srs.handle) == L.ERR_INVALID_ARG
    # the Python surface
    with pytest.raises(k.errors.GenericError):
        kzg.compute_multiproofs(poly, ref_srs, 3)
    with pytest.raises(k.errors.GenericError):
        kzg.compute_multiproofs(poly, ref_srs, 64)
    with pytest.raises(k.errors.SrsCapacityExceeded):
        kzg.compute_multiproofs(k.PolynomialEvalForm(big), ref_srs, 1)
    with pytest.raises(ValueError):                                               # KZG_ERR_INVALID_ARG, as everywhere in the library
        kzg.compute_multiproofs(poly, lag, 1)
    assert np.array_equal(kzg.compute_proof(poly, z, ref_srs), before)
    lag.close()
    other_srs.close()
    other_ctx.close()


# ---- 7. two threads on one context, a second context beside them -----------------------------------------------------------------
def test_threads_and_contexts_at_once(k, test_srs_wire):
    n = 1024
    coeffs = rand_ints(n, 701)
    poly = k.PolynomialCoeffForm(pyref.frs_to_mont(coeffs))
    evals = k.PolynomialEvalForm(pyref.frs_to_mont(pyref.dft(coeffs)))
    ctx_a = k._lib.Context(0)
    ctx_b = k._lib.Context(0)
    srs_a = k.SRS(test_srs_wire[:n], order=n, ctx=ctx_a)
    srs_b = k.SRS(test_srs_wire[:n], order=n, ctx=ctx_b)
    kz_a, kz_b = k.KZG.new(ctx_a), k.KZG.new(ctx_b)
    kz_a.calculate_and_store_roots_of_unity(n * 32)
    roots = kz_a.get_roots_of_unities()
    # expected values, one call at a time, before anything runs concurrently
    ref_srs = k.SRS(test_srs_wire[:n], order=n)
    kz = kzg_for(k, n)
    want_mp = kz.compute_multiproofs(poly, ref_srs, 1)
    want_mp8 = kz.compute_multiproofs(poly, ref_srs, 8)
    want_proof = [kz.compute_proof(evals, roots[i], ref_srs) for i in (0, 5)]
    want_commit = kz.commit_coeff_form(poly, ref_srs)
    ref_srs.close()
    errors, results = [], {}

    def run(name, fn):
        try:
            results[name] = fn()
        except Exception as e:                                      # reported below
            errors.append((name, repr(e)))

    def multi():                                                    # its first call builds the cache on srs_a
        return [kz_a.compute_multiproofs(poly, srs_a, 1) for _ in range(3)]

    def singles():
        return [(kz_a.compute_proof(evals, roots[i % 2 * 5], srs_a), kz_a.commit_coeff_form(poly, srs_a)) for i in range(8)]

    def other():
        return [kz_b.compute_multiproofs(poly, srs_b, 8) for _ in range(3)]

    ts = [threading.Thread(target=run, args=(nm, fn)) for nm, fn in (("multi", multi), ("singles", singles), ("other", other))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert all(np.array_equal(r, want_mp) for r in results["multi"])
    assert all(np.array_equal(r, want_mp8) for r in results["other"])
    for i, (p, c) in enumerate(results["singles"]):
        assert np.array_equal(p, want_proof[i % 2]) and np.array_equal(c, want_commit)
    srs_a.close(); srs_b.close()
    ctx_a.close(); ctx_b.close()


# ---- 8. the bound-checked build runs tests 1-4 with every site counter at 0 -------------------------------------------------------
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
WORKLOAD = ["tests/test_gpu_multiproofs.py::" + t for t in (
    "test_l1_equals_compute_proof_at_every_domain_point", "test_cosets_equal_commitments_of_the_quotients",
    "test_known_tau_values_and_one_pairing", "test_zero_and_constant_polynomials_give_flagged_identities",
    "test_monomial_and_equal_coefficients", "test_eval_form_and_coeff_form_agree")]


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
