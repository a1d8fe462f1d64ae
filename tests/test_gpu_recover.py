"""-m gpu: erasure decoding (`kzg_recover_from_cosets`, `KZG.recover_from_cosets`): a polynomial from a subset of its cosets.  Every
expected value comes from a polynomial the test chose, evaluated with an O(n log n) Python FFT; none comes from the code under test.
Round trips in both output forms over the shapes and missing-coset patterns that take different paths, permuted items, degenerate
polynomials, the consistency flag, the protocol end to end (prove, verify, recover, re-commit), the error table, threads and contexts at
once, and the bound-checked build.  Bit-exact: np.array_equal on the wire words."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

import pyref
import recover_ref
from pyref import R_

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TAU = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/recover/v1").digest(), "big") % R_

# (2048, *): one NTT tile; (4096, *): two NTT passes and the high half of the g-power tables; (65536, 64): m = 1 024, four root tiles
SHAPES = [(2, 1), (4, 1), (8, 4), (64, 4), (2048, 1), (2048, 16), (2048, 1024), (4096, 1), (4096, 64), (65536, 64)]
PATTERNS = ("exact", "all", "one", "odd_missing", "block_missing", "one_missing", "odd_count_missing")


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


def fft_np(vals, inverse=False):
    """recover_ref.fft with the butterflies of a stage as one numpy object-array expression (same values; 2^16 points in a second)."""
    n = len(vals)
    log_n = n.bit_length() - 1
    w = pyref.root_of_unity(log_n)
    if inverse:
        w = pow(w, -1, R_)
    rev = [int(format(i, "0%db" % log_n)[::-1], 2) if log_n else 0 for i in range(n)]
    a = np.array([vals[r] for r in rev], dtype=object)
    h = 1
    while h < n:
        wh = pow(w, n // (2 * h), R_)
        tw = [1] * h
        for t in range(1, h):
            tw[t] = tw[t - 1] * wh % R_
        a = a.reshape(n // (2 * h), 2, h)
        v = a[:, 1, :] * np.array(tw, dtype=object)[None, :] % R_
        a = np.stack([(a[:, 0, :] + v) % R_, (a[:, 0, :] - v) % R_], axis=1).reshape(n)
        h *= 2
    out = [int(x) for x in a]
    if inverse:
        ninv = pow(n, -1, R_)
        out = [x * ninv % R_ for x in out]
    return out


def test_the_fast_fft_is_the_reference_fft():
    for n in (1, 2, 8, 64, 256):
        vals = [random.Random(n).randrange(R_) for _ in range(n)]
        assert fft_np(vals) == recover_ref.fft(vals) and fft_np(vals, True) == recover_ref.fft(vals, True)


def present_cosets(pattern, m, rnd):
    """The cosets a pattern keeps, as a shuffled list (items arrive in any order)."""
    if pattern == "exact":
        ks = rnd.sample(range(m), rnd.randint(1, m))
    elif pattern == "all":
        ks = list(range(m))
    elif pattern == "one":
        ks = [rnd.randrange(m)]
    elif pattern == "odd_missing":
        ks = list(range(0, m, 2))
    elif pattern == "block_missing":
        a, b = m // 4, max(m // 2, 1)
        ks = [kk for kk in range(m) if not a <= kk < a + b]
    elif pattern == "one_missing":
        gone = rnd.randrange(m)
        ks = [kk for kk in range(m) if kk != gone]
    else:                                                           # an odd number of missing cosets, more than one where m allows
        gone = set(rnd.sample(range(m), 3 if m >= 4 else 1))
        ks = [kk for kk in range(m) if kk not in gone]
    rnd.shuffle(ks)
    return ks


def round_trip_cases():
    cases = []
    for n, l in SHAPES:
        seen = set()
        for pattern in PATTERNS:
            ks = present_cosets(pattern, n // l, random.Random("%d/%d/%s" % (n, l, pattern)))
            if frozenset(ks) in seen:                               # m = 2 has two subsets to offer
                continue
            seen.add(frozenset(ks))
            cases.append(pytest.param(n, l, pattern, id="n%d-l%d-%s" % (n, l, pattern)))
    return cases


def make_case(n, l, ks, degree, seed):
    """A random polynomial of `degree` coefficients: (coefficients, evaluations) as wire arrays and the (count, l, 4) values of cosets ks."""
    rnd = random.Random(seed)
    f = [rnd.randrange(R_) for _ in range(degree)] + [0] * (n - degree)
    coeffs, evals = pyref.frs_to_mont(f), pyref.frs_to_mont(fft_np(f))
    rows = evals.reshape(l, n // l, 4).transpose(1, 0, 2)          # KZG.cosets: row k = evals[k::m]
    return f, coeffs, evals, np.ascontiguousarray(rows[list(ks)])


def raw_recover(k, ctx, ys, ks, n, l, bound, eval_form):
    """The C-ABI entry: (status, output, flag); the output and the flag start from a pattern the call has to overwrite."""
    L = k._lib
    ys = np.ascontiguousarray(ys, dtype=np.uint64)
    idx = np.ascontiguousarray(ks, dtype=np.uint64)
    out = np.full((n, 4), 7, dtype=np.uint64)
    flag = C.c_int32(-1)
    rc = L.load().kzg_recover_from_cosets(ctx.handle, L.ptr(ys), L.ptr(idx), len(idx), n, l, bound, eval_form, L.ptr(out), C.byref(flag))
    return rc, out, flag.value


# ---- 1. round trips, both output forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,l,pattern", round_trip_cases())
def test_round_trip(k, n, l, pattern):
    ks = present_cosets(pattern, n // l, random.Random("%d/%d/%s" % (n, l, pattern)))
    _, coeffs, evals, ys = make_case(n, l, ks, len(ks) * l, "%d/%d/%s/f" % (n, l, pattern))      # exactly count l = deg + 1
    kzg = k.KZG.new()
    got = kzg.recover_from_cosets(ks, ys, n)
    assert isinstance(got, k.PolynomialEvalForm) and np.array_equal(got.evaluations(), evals)
    got = kzg.recover_from_cosets(ks, ys, n, eval_form=False)
    assert isinstance(got, k.PolynomialCoeffForm) and np.array_equal(got.coeffs(), coeffs)
    rc, out, flag = raw_recover(k, k.default_context(), ys, ks, n, l, 0, 1)
    assert (rc, flag) == (0, 1) and np.array_equal(out, evals)


# ---- 2. the order of the items does not matter -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,l", [(64, 4), (4096, 16)])
def test_permuted_items_give_identical_bits(k, n, l):
    m = n // l
    rnd = random.Random(n)
    ks = sorted(rnd.sample(range(m), m // 2 + 1))
    _, coeffs, evals, ys = make_case(n, l, ks, len(ks) * l, n + 1)
    ctx = k.default_context()
    for form, want in ((1, evals), (0, coeffs)):
        for _ in range(3):
            perm = list(range(len(ks)))
            rnd.shuffle(perm)
            rc, out, flag = raw_recover(k, ctx, ys[perm], [ks[i] for i in perm], n, l, 0, form)
            assert (rc, flag) == (0, 1) and np.array_equal(out, want)


# ---- 3. the zero polynomial and a constant -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,l", [(8, 4), (64, 4), (4096, 1)])
def test_zero_and_constant_polynomials(k, n, l):
    m = n // l
    ks = random.Random(n + l).sample(range(m), max(m // 2, 1))
    ctx = k.default_context()
    zero = np.zeros((len(ks), l, 4), dtype=np.uint64)
    for form in (0, 1):
        rc, out, flag = raw_recover(k, ctx, zero, ks, n, l, 1, form)              # bound 1: every coefficient but the constant term is checked
        assert (rc, flag) == (0, 1) and not out.any()
    c = pyref.fr_to_mont(0x1234567)
    const = np.broadcast_to(c, (len(ks), l, 4))
    rc, out, flag = raw_recover(k, ctx, const, ks, n, l, 1, 1)
    assert (rc, flag) == (0, 1) and np.array_equal(out, np.broadcast_to(c, (n, 4)))
    rc, out, flag = raw_recover(k, ctx, const, ks, n, l, 1, 0)
    assert (rc, flag) == (0, 1) and np.array_equal(out[0], c) and not out[1:].any()


# ---- 4. the consistency flag -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,l,count", [(64, 4, 8), (4096, 16, 100)])
def test_consistency_flag(k, n, l, count):
    m = n // l
    d = count * l
    ks = random.Random(n + count).sample(range(m), count)
    f, coeffs, evals, ys = make_case(n, l, ks, d // 2, n + 2)                        # degree < count l / 2: twice the cosets it needs
    ctx = k.default_context()
    kzg = k.KZG.new()
    for form, want in ((1, evals), (0, coeffs)):
        rc, out, flag = raw_recover(k, ctx, ys, ks, n, l, d // 2, form)
        assert (rc, flag) == (0, 1) and np.array_equal(out, want)
    assert np.array_equal(kzg.recover_from_cosets(ks, ys, n, degree_bound=d // 2).evaluations(), evals)
    bad = ys.copy()
    bad[count // 2, l - 1] = pyref.fr_to_mont(pyref.fr_from_mont(bad[count // 2, l - 1]) + 1)       # one value changed
    rc, out_c, flag = raw_recover(k, ctx, bad, ks, n, l, d // 2, 0)
    assert (rc, flag) == (0, 0)
    assert not out_c[d:].any()                                                        # still of degree < count l
    rc, out_e, flag = raw_recover(k, ctx, bad, ks, n, l, d // 2, 1)
    assert (rc, flag) == (0, 0)
    rows = kzg.cosets(k.PolynomialEvalForm(out_e), l)
    assert np.array_equal(rows[ks], bad)                                              # ... and still through the given values
    rc, out, flag = raw_recover(k, ctx, bad, ks, n, l, 0, 0)                          # no bound: the same interpolant, flag 1
    assert (rc, flag) == (0, 1) and np.array_equal(out, out_c)
    rc, out, flag = raw_recover(k, ctx, bad, ks, n, l, d, 0)
    assert (rc, flag) == (0, 1) and np.array_equal(out, out_c)
    with pytest.raises(k.errors.GenericError, match="degree bound"):
        kzg.recover_from_cosets(ks, bad, n, degree_bound=d // 2)
    if n == 64:
        bad_ints = [[pyref.fr_from_mont(v) for v in row] for row in bad]
        want, consistent = recover_ref.recover(n, l, ks, bad_ints, d // 2)
        assert not consistent and np.array_equal(out_c, pyref.frs_to_mont(want))
        assert np.array_equal(out_e, pyref.frs_to_mont(recover_ref.fft(want)))
    L = k._lib                                                                        # out_consistent = NULL is allowed
    out = np.zeros((n, 4), dtype=np.uint64)
    idx = np.ascontiguousarray(ks, dtype=np.uint64)
    assert L.load().kzg_recover_from_cosets(ctx.handle, L.ptr(bad), L.ptr(idx), count, n, l, d // 2, 0, L.ptr(out), None) == 0
    assert np.array_equal(out, out_c)


# ---- 5. the protocol end to end: prove, sample, verify, recover, re-commit ---------------------------------------------------------
def test_end_to_end_with_proofs(k):
    n, l = 4096, 16
    m = n // l
    rnd = random.Random(55)
    f = [rnd.randrange(R_) for _ in range(n // 2)] + [0] * (n // 2)                   # the rate-1/2 extension of n / 2 coefficients
    poly = k.PolynomialEvalForm(pyref.frs_to_mont(fft_np(f)))
    srs = k.SRS.generate(TAU, n)
    kzg = k.KZG.new()
    commitment = kzg.commit_eval_form(poly, srs)
    proofs = kzg.compute_multiproofs(poly, srs, l)
    cosets = kzg.cosets(poly, l)
    ks = rnd.sample(range(m), m // 2)
    ys = np.ascontiguousarray(cosets[ks])
    g2 = k.helpers.g2_mul_generator(k.fr.fr_from_int(pow(TAU, l, R_)))
    assert k.verifier.verify_multiproof_batch([commitment], [0] * len(ks), ks, ys, [proofs[kk] for kk in ks], n, srs, g2) is True
    got = kzg.recover_from_cosets(ks, ys, n, degree_bound=n // 2)
    assert np.array_equal(got.evaluations(), poly.evaluations())
    assert np.array_equal(kzg.commit_eval_form(got, srs), commitment)
    coeffs = kzg.recover_from_cosets(ks, ys, n, degree_bound=n // 2, eval_form=False)
    assert np.array_equal(coeffs.coeffs(), pyref.frs_to_mont(f))
    assert np.array_equal(kzg.commit_coeff_form(coeffs, srs), commitment)
    srs.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------
def test_error_table_then_a_bit_exact_call(k):
    L = k._lib
    lib = L.load()
    ctx = L.Context(0)
    n, l = 64, 4
    m = n // l
    ks = [3, 0, 9, 14, 5]
    _, coeffs, evals, ys = make_case(n, l, ks, len(ks) * l, 606)
    out = np.zeros((n, 4), dtype=np.uint64)
    flag = C.c_int32(0)

    def call(idx, n_=n, l_=l, bound=0, ctx_h=ctx.handle, ys_=ys, out_=out, null_idx=False, count=None):
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        return lib.kzg_recover_from_cosets(ctx_h, None if ys_ is None else L.ptr(ys_), None if null_idx else L.ptr(idx),
                                           len(idx) if count is None else count, n_, l_, bound, 0, None if out_ is None else L.ptr(out_), C.byref(flag))

    assert call(ks, ctx_h=None) == L.ERR_INVALID_ARG                                   # 1. null pointers, in front of everything
    assert call(ks, ys_=None, n_=0) == L.ERR_INVALID_ARG
    assert call(ks, null_idx=True, n_=96) == L.ERR_INVALID_ARG
    assert call(ks, out_=None, n_=1 << 25) == L.ERR_INVALID_ARG
    assert call(ks, n_=0) == L.ERR_NOT_POWER_OF_TWO                                    # 2.
    assert call(ks, n_=96, l_=3) == L.ERR_NOT_POWER_OF_TWO
    assert call(ks, n_=1 << 25, l_=3) == L.ERR_DOMAIN                                  # 3.
    assert call(ks, n_=1) == L.ERR_INVALID_ARG                                         # 4.
    assert call(ks, l_=0) == L.ERR_INVALID_ARG
    assert call(ks, l_=3) == L.ERR_INVALID_ARG
    assert call(ks, l_=64) == L.ERR_INVALID_ARG
    assert call(ks, count=0) == L.ERR_INVALID_ARG                                      # 5.
    assert call(list(range(m)) + [0]) == L.ERR_INVALID_ARG
    assert call([3, 0, m, 14, 5]) == L.ERR_INVALID_ARG                                 # 6. an index = m
    assert call([3, 0, 2 ** 64 - 1, 14, 5]) == L.ERR_INVALID_ARG
    assert call([3, 0, 9, 3, 5]) == L.ERR_INVALID_ARG                                  #    a duplicate
    assert call(ks, bound=len(ks) * l + 1) == L.ERR_INVALID_ARG                        # 7. too few cosets
    one = np.zeros((1, 1, 4), dtype=np.uint64)                                        # 8. the cap: refused before anything is allocated or read
    assert call([0], n_=1 << 24, l_=1, ys_=one, out_=one.reshape(1, 4)) == L.ERR_TOO_LARGE
    assert call([0], n_=1 << 24, l_=1, bound=2, ys_=one, out_=one.reshape(1, 4)) == L.ERR_INVALID_ARG      # 7 in front of 8
    assert not out.any()
    # the Python surface
    kzg = k.KZG.new(ctx)
    for bad_ks in ([3, 0, m, 14, 5], [3, 0, 9, 3, 5]):
        with pytest.raises(k.errors.GenericError):
            kzg.recover_from_cosets(bad_ks, ys, n)
    with pytest.raises(k.errors.GenericError):
        kzg.recover_from_cosets(ks, ys, n, degree_bound=len(ks) * l + 1)
    # the context is as usable as before
    assert call(ks) == 0 and flag.value == 1 and np.array_equal(out, coeffs)
    assert np.array_equal(kzg.recover_from_cosets(ks, ys, n).evaluations(), evals)
    ctx.close()


# ---- 7. two threads on one context, a second context beside them -------------------------------------------------------------------
def test_threads_and_contexts_at_once(k):
    cases = {}
    for name, (n, l, count) in {"a": (1024, 4, 130), "b": (512, 1, 300), "c": (2048, 32, 33)}.items():
        ks = random.Random(name).sample(range(n // l), count)
        _, coeffs, evals, ys = make_case(n, l, ks, count * l, "threads/" + name)
        cases[name] = (n, l, ks, ys, coeffs, evals)
    ctx_a, ctx_b = k._lib.Context(0), k._lib.Context(0)
    kz_a, kz_b = k.KZG.new(ctx_a), k.KZG.new(ctx_b)
    errors, results = [], {}

    def run(name, kz, eval_form):
        try:
            n, l, ks, ys = cases[name][:4]
            res = [kz.recover_from_cosets(ks, ys, n, eval_form=eval_form) for _ in range(4)]
            results[name] = [r.evaluations() if eval_form else r.coeffs() for r in res]
        except Exception as e:                                      # reported below
            errors.append((name, repr(e)))

    ts = [threading.Thread(target=run, args=a) for a in (("a", kz_a, True), ("b", kz_a, False), ("c", kz_b, True))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert all(np.array_equal(r, cases["a"][5]) for r in results["a"])
    assert all(np.array_equal(r, cases["b"][4]) for r in results["b"])
    assert all(np.array_equal(r, cases["c"][5]) for r in results["c"])
    ctx_a.close(); ctx_b.close()


# ---- 8. the bound-checked build runs the round trips of n <= 4096 with every site counter at 0 -------------------------------------
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
rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", "-x", "tests/test_gpu_recover.py::test_round_trip", "-k", "not n65536"])
counts = (C.c_ulonglong * n)()
first = (C.c_int32 * (9 * n))()
assert h.kzg_bc_read_all(counts, first) == 0
print("PYTEST_RC", int(rc))
for s in range(n):
    print("SITE", s, counts[s])
'''


def test_bound_checked_build_keeps_every_precondition():
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "PYTEST_RC 0" in out, (out[-3000:], res.stderr[-2000:])
    assert " passed" in out and "no tests ran" not in out, out[-1000:]
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert sites
    fired = {int(s[1]): int(s[2]) for s in sites if int(s[2])}
    assert not fired, fired
