"""-m gpu: the G2 MSM on the device (`kzg_msm_g2`, csrc/g2msm.hip) against closed forms.  Bases are [s_i] G2 from the host's fixed-base
multiplication (`kzg_g2_mul_generator`) with known s_i, so the expected result is [sum a_i s_i mod r] G2 from the same call, compared bit
for bit: sizes around the wave, workgroup and plan boundaries (window bits change at 2 048 and 4 096 pairs), scalar sets at the edges of
the signed-digit recoding, degenerate base sets (all equal: the buckets double; P and -P: they cancel; identities mixed in), the error
paths, and bit-identical repeats on a second context."""
import ctypes as C
import random

import numpy as np
import pytest

import rust_kzg_bn254_amd as k
from pyref import P, R_
from rust_kzg_bn254_amd import _lib, helpers
from rust_kzg_bn254_amd.errors import MsmError, NotOnCurveError
from rust_kzg_bn254_amd.fr import fr_from_int, frs_from_ints

pytestmark = pytest.mark.gpu

NMAX = 4096
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 2047, 2048, 4095, 4096]      # 2 048 and 4 096: generic_window goes 4 -> 5 -> 6 bits


def plan_c(n):
    """csrc/msm_plan.h generic_window(n, 1)"""
    return min(14, max(4, n.bit_length() - 1 - 6))


@pytest.fixture(scope="module")
def pool():
    """NMAX bases [s_i] G2 with known s_i (computed once, never modified)"""
    rnd = random.Random(2024)
    s = [rnd.randrange(1, R_) for _ in range(NMAX)]
    pts = np.stack([helpers.g2_mul_generator(fr_from_int(v)) for v in s])
    pts.setflags(write=False)
    return s, pts


def expect(s, a):
    return helpers.g2_mul_generator(fr_from_int(sum(x * y for x, y in zip(s, a)) % R_))


def neg(p):
    q = np.array(p, dtype=np.uint64)
    for c in (2, 3):
        v = sum(int(q[4 * c + j]) << (64 * j) for j in range(4))
        v = (P - v) % P
        for j in range(4):
            q[4 * c + j] = (v >> (64 * j)) & (2 ** 64 - 1)
    return q


def msm(pts, a, ctx=None):
    return helpers.msm_g2(pts, frs_from_ints(a), ctx=ctx)


@pytest.mark.parametrize("n", SIZES)
def test_random_scalars_at_every_size(pool, n):
    s, pts = pool
    rnd = random.Random(n)
    a = [rnd.randrange(R_) for _ in range(n)]
    got = msm(pts[:n], a)
    assert np.array_equal(got, expect(s[:n], a))
    assert got.any()


@pytest.mark.parametrize("n", [65, 257, 2048])
def test_scalar_sets_at_the_edges_of_the_recoding(pool, n):
    s, pts = pool
    c = plan_c(n)
    rnd = random.Random(100 + n)
    sets = {"ones": [1] * n, "r-1": [R_ - 1] * n, "equal": [rnd.randrange(R_)] * n}
    for kk in (1, 2, 7, 253 // c):                                           # digits at the sign-carry edge of window kk
        sets["2^(ck)-1 k=%d" % kk] = [(1 << (c * kk)) - 1] * n
        sets["2^(ck) k=%d" % kk] = [1 << (c * kk)] * n
        sets["2^(ck-1) k=%d" % kk] = [1 << (c * kk - 1)] * n
    sets["mixed edges"] = [rnd.choice([(1 << (c * j)) - 1, 1 << (c * j), 1 << (c * j - 1), R_ - 1, 0, 1]) for j in range(1, n + 1)]
    sets["mixed edges"] = [v % R_ for v in sets["mixed edges"]]
    for name, a in sets.items():
        assert np.array_equal(msm(pts[:n], a), expect(s[:n], a)), name
    # all zero: the identity, flag set
    out = np.zeros(16, np.uint64); inf = C.c_uint8(0)
    z = frs_from_ints([0] * n)
    p_ = np.ascontiguousarray(pts[:n])
    ctx = _lib.default_context()
    assert _lib.load().kzg_msm_g2(ctx.handle, _lib.ptr(p_), n, _lib.ptr(z), n, _lib.ptr(out), C.byref(inf)) == _lib.OK
    assert inf.value == 1 and not out.any()


def test_degenerate_base_sets(pool):
    s, pts = pool
    rnd = random.Random(7)
    n = 300
    a = [rnd.randrange(R_) for _ in range(n)]
    # all bases equal: every bucket meets P + P
    same = np.repeat(pts[5:6], n, axis=0)
    assert np.array_equal(msm(same, a), expect([s[5]] * n, a))
    assert np.array_equal(msm(same, [3] * n), expect([s[5]], [3 * n]))
    # P and -P alternating with equal scalars: everything cancels
    alt = np.stack([pts[9] if i % 2 == 0 else neg(pts[9]) for i in range(n)])
    assert not msm(alt, [a[0]] * n).any()
    assert not msm(alt, [1] * n).any()
    # ... and with one extra P the sum is that term
    alt3 = np.concatenate([alt, pts[9:10]])
    assert np.array_equal(msm(alt3, [a[0]] * (n + 1)), expect([s[9]], [a[0]]))
    # identity bases mixed in (skipped), also first and last
    mixed = np.array(pts[:n])
    dead = [0, 1, 63, 64, 100, 299]
    mixed[dead] = 0
    keep = [i for i in range(n) if i not in dead]
    assert np.array_equal(msm(mixed, a), expect([s[i] for i in keep], [a[i] for i in keep]))
    assert not msm(np.zeros((4, 16), np.uint64), [1, 2, 3, 4]).any()


def test_errors_and_empty_input(pool):
    s, pts = pool
    ctx = _lib.default_context()
    lib = _lib.load()
    off = np.array(pts[:40])
    off[17, 0] ^= np.uint64(1)
    with pytest.raises(NotOnCurveError):
        msm(off, [1] * 40)
    assert "17" in ctx.last_error()
    with pytest.raises(MsmError):
        helpers.msm_g2(pts[:5], frs_from_ints([1, 2, 3, 4]))
    out = np.zeros(16, np.uint64); inf = C.c_uint8(0)
    sc = frs_from_ints([1, 2, 3])
    p3 = np.ascontiguousarray(pts[:3])
    assert lib.kzg_msm_g2(ctx.handle, None, 3, _lib.ptr(sc), 3, _lib.ptr(out), C.byref(inf)) == _lib.ERR_INVALID_ARG
    assert lib.kzg_msm_g2(ctx.handle, _lib.ptr(p3), 3, None, 3, _lib.ptr(out), C.byref(inf)) == _lib.ERR_INVALID_ARG
    assert lib.kzg_msm_g2(ctx.handle, _lib.ptr(p3), 3, _lib.ptr(sc), 3, None, C.byref(inf)) == _lib.ERR_INVALID_ARG
    assert lib.kzg_msm_g2(None, _lib.ptr(p3), 3, _lib.ptr(sc), 3, _lib.ptr(out), C.byref(inf)) == _lib.ERR_INVALID_ARG
    assert lib.kzg_msm_g2(ctx.handle, _lib.ptr(p3), 3, _lib.ptr(sc), 2, _lib.ptr(out), C.byref(inf)) == _lib.ERR_MSM_LENGTH_MISMATCH
    out[:] = 1
    assert lib.kzg_msm_g2(ctx.handle, None, 0, None, 0, _lib.ptr(out), C.byref(inf)) == _lib.OK and inf.value == 1 and not out.any()
    # the context stays usable after every error
    assert np.array_equal(msm(pts[:3], [1, 2, 3]), expect(s[:3], [1, 2, 3]))


def test_bit_identical_repeats_and_second_context(pool):
    s, pts = pool
    rnd = random.Random(8)
    n = 1000
    a = [rnd.randrange(R_) for _ in range(n)]
    first = msm(pts[:n], a)
    assert np.array_equal(first, expect(s[:n], a))
    for _ in range(2):
        assert np.array_equal(msm(pts[:n], a), first)
    other = k.Context(0)
    try:
        assert np.array_equal(msm(pts[:n], a, ctx=other), first)
        assert np.array_equal(msm(pts[:n], a, ctx=other), first)
    finally:
        other.close()
