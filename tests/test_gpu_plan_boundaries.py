"""-m gpu: commitments at the planner's mode boundaries (csrc/msm_plan.h, engine.h srs_bases) on a known-tau SRS of 2^15 points:
4096 | 4097 (bit sums -> the c = 15 window tables), 8192 | 8193 (their last size -> the c = 17 tables) and 16383 | 16384 (-> NAF digits over
the per-bit tables), each once alone (reduction on lane quads) and once with another MSM in flight on a second slot (lane pairs); and two
batched launches (64 buckets per polynomial; whole units of 4 096 buckets per polynomial).  Every result against (sum_i s_i tau^i) G by
big-integer arithmetic."""
import ctypes as C
import random

import numpy as np
import pytest

import pyref
from pyref import R_

pytestmark = pytest.mark.gpu

TAU = int.from_bytes(__import__("hashlib").sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % R_
LENGTHS = [4096, 4097, 8192, 8193, 16383, 16384]


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


@pytest.fixture(scope="module")
def tau_srs(k):
    s = k.SRS.generate(TAU, 1 << 15)
    yield s
    s.close()


@pytest.fixture(scope="module")
def tau_powers():
    out, t = [], 1
    for _ in range(1 << 14):
        out.append(t)
        t = t * TAU % R_
    return out


def scalars(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R_) for _ in range(n)]


def expected(values, tau_powers):
    s = sum(c * t for c, t in zip(values, tau_powers)) % R_
    return pyref.ec_mul(s, (1, 2)) if s else None


def begin(k, srs, mont, slot):
    from rust_kzg_bn254_amd import _lib
    rc = _lib.load().kzg_msm_g1_srs_begin(k.default_context().handle, srs.handle, 0, _lib.ptr(mont), len(mont), slot)
    assert rc == _lib.OK, rc


def end(k, slot):
    from rust_kzg_bn254_amd import _lib
    out = np.zeros(8, dtype=np.uint64)
    inf = C.c_uint8(0)
    rc = _lib.load().kzg_msm_g1_srs_end(k.default_context().handle, slot, _lib.ptr(out), C.byref(inf), None)
    assert rc == _lib.OK, rc
    return pyref.point_from_wire(out)


@pytest.mark.parametrize("n", LENGTHS)
def test_commitment_alone_and_beside_another_msm(k, tau_srs, tau_powers, n):
    values = scalars(n, 4000 + n)
    mont = np.ascontiguousarray(pyref.frs_to_mont(values), dtype=np.uint64)
    want = expected(values, tau_powers)
    begin(k, tau_srs, mont, 0)                       # nothing else in flight: planned alone
    assert end(k, 0) == want, (n, "alone")
    other_values = scalars(5000, 77)
    other = np.ascontiguousarray(pyref.frs_to_mont(other_values), dtype=np.uint64)
    begin(k, tau_srs, other, 1)
    try:
        begin(k, tau_srs, mont, 0)                   # slot 1 in flight: planned beside another MSM
        got = end(k, 0)
    finally:
        got_other = end(k, 1)
    assert got == want, (n, "beside another MSM")
    assert got_other == expected(other_values, tau_powers)


@pytest.mark.parametrize("count,n", [(3, 64), (2, 1 << 13)])
def test_batched_launch(k, tau_srs, tau_powers, count, n):
    kzg = k.KZG.new()
    rows = [scalars(n, 9000 + 10 * n + j) for j in range(count)]
    got = kzg.commit_coeff_form_batch([k.PolynomialCoeffForm(pyref.frs_to_mont(v)) for v in rows], tau_srs)
    assert got.shape == (count, 8)
    for j, v in enumerate(rows):
        assert pyref.point_from_wire(got[j]) == expected(v, tau_powers), (count, n, j)
