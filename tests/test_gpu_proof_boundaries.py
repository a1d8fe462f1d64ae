"""-m gpu: proofs and evaluations at the sizes on either side of every threshold of the proof plan (csrc/proof_plan.h), on a known-tau SRS of 2^14
points: 2^9 | 2^10 (the one-workgroup inversion chain alone | chained levels; with host evaluations also the chain on the main | auxiliary
stream), 2^11 | 2^12 (no x4 level | one), 2^10 | 2^11 (one | several workgroups for the barycentric sum), 2^12 | 2^13 (the known-index table |
the generic on-domain path), and 1, 2 and 4 points.  Each size at one z off the domain and at z = w^m for m in {0, n/2 + 1, n - 1}, through the
synchronous call, kzg_compute_proof_begin / _end on slot 1 and the evaluation-only call; 2^10 and 2^12 once more with a cached Lagrange basis of
exactly n points (the quotient committed in evaluation form, no inverse NTT).  Expected values by big integers: y from the barycentric formula
(the stored evaluation on the domain), proof = ((f(tau) - y) / (tau - z)) G1."""
import ctypes as C
import functools
import hashlib
import random

import numpy as np
import pytest

import pyref
from pyref import R_

pytestmark = pytest.mark.gpu

TAU = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % R_
MONT = (1 << 256) % R_
LOGS = [0, 1, 2, 9, 10, 11, 12, 13, 14]


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


@pytest.fixture(scope="module")
def srs14(k):
    s = k.SRS.generate(TAU, 1 << 14)
    yield s
    s.close()


def evaluate(evals, roots, x):
    """(x^n - 1)/n * sum_i f_i w^i / (x - w^i), x off the domain (primitives/src/helpers.rs:507-532); one inversion"""
    n = len(evals)
    dens = [(x - w) % R_ for w in roots]
    pre, acc = [], 1
    for d in dens:
        pre.append(acc)
        acc = acc * d % R_
    inv = pow(acc, -1, R_)
    tot = 0
    for i in range(n - 1, -1, -1):
        tot += evals[i] * roots[i] % R_ * (inv * pre[i] % R_)
        inv = inv * dens[i] % R_
    return tot % R_ * (pow(x, n, R_) - 1) % R_ * pow(n, -1, R_) % R_


@functools.lru_cache(maxsize=None)
def reference(log_n):
    """evaluations (Montgomery words) and, per point z: (z, y, the proof as an affine point or None for the identity); computed once per size"""
    n = 1 << log_n
    rnd = random.Random(0xB0DA + log_n)
    evals = [rnd.randrange(R_) for _ in range(n)]
    w = pyref.root_of_unity(log_n) if log_n else 1
    roots, cur = [], 1
    for _ in range(n):
        roots.append(cur)
        cur = cur * w % R_
    ftau = evaluate(evals, roots, TAU)
    z_off = rnd.randrange(R_)
    points = [(z_off, evaluate(evals, roots, z_off))] + [(roots[m], evals[m]) for m in sorted({0, (n // 2 + 1) % n, n - 1})]
    cases = []
    for z, y in points:
        q = (ftau - y) * pow(TAU - z, -1, R_) % R_
        cases.append((z, y, pyref.ec_mul(q, (1, 2)) if q else None))
    words = np.frombuffer(b"".join((v * MONT % R_).to_bytes(32, "little") for v in evals), dtype=np.uint64).reshape(-1, 4).copy()
    return words, cases


def check_point(out, inf, want, what):
    if want is None:
        assert inf == 1 and not out.any(), what
    else:
        assert inf == 0 and pyref.point_from_wire(out) == want, what


def prove_both_ways(k, srs, log_n, tag):
    """every point of the size through the synchronous call and through begin / end on slot 1"""
    words, cases = reference(log_n)
    n = 1 << log_n
    ctx = k.default_context(); lib = k._lib.load()
    kzg = k.KZG.new(); kzg.calculate_and_store_roots_of_unity(n * 32)
    for i, (z, y_want, pt_want) in enumerate(cases):
        zw = pyref.fr_to_mont(z)
        out = np.zeros(8, dtype=np.uint64); inf = C.c_uint8(0); y = np.zeros(4, dtype=np.uint64)
        roots = k._lib.as_u64(kzg.expanded_roots_of_unity, 4)
        assert lib.kzg_compute_proof(ctx.handle, srs.handle, k._lib.ptr(words), n, k._lib.ptr(roots), len(roots), k._lib.ptr(zw), k._lib.ptr(out), C.byref(inf), k._lib.ptr(y)) == 0
        assert pyref.fr_from_mont(y) == y_want, (tag, log_n, i, "sync y")
        check_point(out, inf.value, pt_want, (tag, log_n, i, "sync proof"))
        out = np.zeros(8, dtype=np.uint64); inf = C.c_uint8(0); y = np.zeros(4, dtype=np.uint64)
        assert lib.kzg_compute_proof_begin(ctx.handle, srs.handle, k._lib.ptr(words), n, None, n, k._lib.ptr(zw), 1) == 0
        assert lib.kzg_compute_proof_end(ctx.handle, 1, k._lib.ptr(out), C.byref(inf), k._lib.ptr(y)) == 0
        assert pyref.fr_from_mont(y) == y_want, (tag, log_n, i, "slot 1 y")
        check_point(out, inf.value, pt_want, (tag, log_n, i, "slot 1 proof"))


@pytest.mark.parametrize("log_n", LOGS)
def test_proofs_either_side_of_every_plan_threshold(k, srs14, log_n):
    prove_both_ways(k, srs14, log_n, "monomial")


@pytest.mark.parametrize("log_n", LOGS)
def test_evaluation_only_either_side_of_every_plan_threshold(k, log_n):
    words, cases = reference(log_n)
    ctx = k.default_context(); lib = k._lib.load()
    for i, (z, y_want, _) in enumerate(cases):
        zw = pyref.fr_to_mont(z)
        y = np.zeros(4, dtype=np.uint64)
        assert lib.kzg_evaluate_polynomial_in_evaluation_form(ctx.handle, k._lib.ptr(words), 1 << log_n, k._lib.ptr(zw), k._lib.ptr(y)) == 0
        assert pyref.fr_from_mont(y) == y_want, (log_n, i)


@pytest.mark.parametrize("log_n", [10, 12])
def test_proofs_over_a_cached_lagrange_basis(k, srs14, log_n):
    """a Lagrange basis of exactly n points cached with the SRS: the quotient's evaluations are committed as they are, the inverse NTT is skipped"""
    srs14.cache_lagrange(1 << log_n)
    try:
        prove_both_ways(k, srs14, log_n, "lagrange")
    finally:
        srs14.drop_lagrange()
