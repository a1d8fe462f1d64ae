"""-m gpu: the device-resident G2 SRS (`kzg_g2srs_*`) and the G2 commitments over it, against closed forms for a known tau: generated
points equal [tau^k] G2 of the host's fixed-base multiplication bit for bit and pair with the G1 SRS of the same tau; commitments of 2^12
and 2^16 coefficients or evaluations equal [f(tau)] G2 and pair with the G1 commitment -- also for the adversarial shape (all coefficients
equal: every window has ONE bucket with all the entries), which runs in the same time as the random one because the accumulate kernel
splits the sorted entries equally; a nonzero offset and device-resident scalars equal the host-buffer call."""
import ctypes as C
import random
import time

import numpy as np
import pytest

import rust_kzg_bn254_amd as k
from pyref import R_
from rust_kzg_bn254_amd import _lib, helpers
from rust_kzg_bn254_amd.errors import NotOnCurveError, SerializationError, SrsCapacityExceeded
from rust_kzg_bn254_amd.fr import fr_from_int, frs_from_ints

pytestmark = pytest.mark.gpu
TAU = 0x1D2C3B4A5968778695A4B3C2D1E0F1234567


def tau_g2(e):
    return helpers.g2_mul_generator(fr_from_int(pow(TAU, e, R_)))


def horner(coeffs):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * TAU + c) % R_
    return acc


@pytest.fixture(scope="module")
def srs16():
    """[tau^i]_2 and [tau^i]_1 for i < 2^16, generated once"""
    g2 = k.G2SRS.generate(TAU, 1 << 16)
    g1 = k.SRS.generate(TAU, 1 << 16)
    yield g1, g2
    g2.close(); g1.close()


@pytest.mark.parametrize("n,first", [(65, 0), (65, 12345), (4097, 0), (4097, 12345)])
def test_generate_against_the_fixed_base_multiplication(n, first):
    srs = k.G2SRS.generate(TAU, n, first_power=first)
    try:
        assert len(srs) == n
        pts = srs.g2
        for i in sorted({0, 1, 63, 64, min(65, n - 1), n - 1}):
            assert np.array_equal(pts[i], tau_g2(first + i)), i
        # every point passes the upload check; the copy downloads to the same bits
        again = k.G2SRS.from_points(pts)
        try:
            assert np.array_equal(again.g2, pts)
        finally:
            again.close()
        g1 = k.SRS.generate(TAU, 3, first_power=first + n - 3).g1
        G1 = k.SRS.generate(TAU, 1).g1[0]
        for j in range(3):
            assert helpers.pairings_verify(g1[j], helpers.g2_generator(), G1, pts[n - 3 + j])
        assert not helpers.pairings_verify(g1[0], helpers.g2_generator(), G1, pts[n - 2])
    finally:
        srs.close()


def test_upload_rejects_a_point_off_the_twist_with_its_index():
    pts = np.stack([tau_g2(i) for i in range(70)])
    pts[3] = 0                                           # the identity is accepted
    ok = k.G2SRS.from_points(pts)
    assert np.array_equal(ok.g2, pts)
    ok.close()
    bad = pts.copy()
    bad[66, 9] ^= np.uint64(4)
    bad[68, 1] ^= np.uint64(1)
    ctx = _lib.default_context()
    h = C.c_void_p(); idx = C.c_uint64(0)
    assert _lib.load().kzg_g2srs_upload(ctx.handle, _lib.ptr(bad), 70, C.byref(h), C.byref(idx)) == _lib.ERR_NOT_ON_CURVE
    assert idx.value == 66 and not h.value
    with pytest.raises(NotOnCurveError):
        k.G2SRS.from_points(bad)
    empty = k.G2SRS.from_points(np.zeros((0, 16), np.uint64))
    assert len(empty) == 0 and empty.g2.shape == (0, 16)
    empty.close()


def _check_commitments(srs16, coeffs):
    g1, g2 = srs16
    n = len(coeffs)
    kzg = k.KZG.new()
    poly = k.PolynomialCoeffForm(frs_from_ints(coeffs))
    want = helpers.g2_mul_generator(fr_from_int(horner(coeffs)))
    c2 = kzg.commit_g2_coeff_form(poly, g2)
    assert np.array_equal(c2, want)
    c1 = kzg.commit_coeff_form(poly, g1)
    G1 = k.SRS.generate(TAU, 1).g1[0]                           # [tau^0]_1
    assert helpers.pairings_verify(c1, helpers.g2_generator(), G1, c2)
    return c2


@pytest.mark.parametrize("log_n", [12, 16])
def test_known_tau_commitments_coefficient_and_evaluation_form(srs16, log_n):
    n = 1 << log_n
    rnd = random.Random(log_n)
    coeffs = [rnd.randrange(R_) for _ in range(n)]
    c2 = _check_commitments(srs16, coeffs)
    # evaluation form: the same polynomial through the device's own forward transform
    ctx = _lib.default_context()
    ev = np.ascontiguousarray(frs_from_ints(coeffs))
    assert _lib.load().kzg_fr_ntt(ctx.handle, _lib.ptr(ev), n, 0) == _lib.OK
    got = k.KZG.new().commit_g2_eval_form(k.PolynomialEvalForm(ev), srs16[1])
    assert np.array_equal(got, c2)


def test_adversarial_all_equal_coefficients_take_no_longer_than_random_ones(srs16):
    """All coefficients equal: every window's entries fall into ONE bucket.  A lane per bucket would serialise 2^16 additions; the equal
    split keeps the accumulate kernel's work per lane at ceil(entries / lanes).  Both shapes run under the same time limit."""
    n = 1 << 16
    rnd = random.Random(99)
    limit = 5.0
    for coeffs in ([rnd.randrange(R_) for _ in range(n)], [rnd.randrange(R_)] * n, [1] * n):
        t0 = time.perf_counter()
        _check_commitments(srs16, coeffs)
        dt = time.perf_counter() - t0
        print("  2^16 coefficients, %s: %.2f s with its checks" % ("equal" if coeffs[0] == coeffs[1] else "random", dt))
        assert dt < limit


def test_offset_and_device_scalars_equal_the_host_call(srs16):
    import torch
    _, g2 = srs16
    ctx = _lib.default_context()
    lib = _lib.load()
    rnd = random.Random(5)
    n, off = 3000, 12345
    a = [rnd.randrange(R_) for _ in range(n)]
    sc = np.ascontiguousarray(frs_from_ints(a))
    want = helpers.g2_mul_generator(fr_from_int(horner(a) * pow(TAU, off, R_) % R_))
    out = np.zeros(16, np.uint64); inf = C.c_uint8(0)
    assert lib.kzg_msm_g2_srs(ctx.handle, g2.handle, off, _lib.ptr(sc), n, _lib.ptr(out), C.byref(inf)) == _lib.OK
    assert np.array_equal(out, want) and inf.value == 0
    dev = torch.from_numpy(sc.view(np.int64)).cuda()
    out2 = np.zeros(16, np.uint64)
    assert lib.kzg_msm_g2_srs_device(ctx.handle, g2.handle, off, C.c_void_p(dev.data_ptr()), n, _lib.ptr(out2), C.byref(inf)) == _lib.OK
    assert np.array_equal(out2, want)
    # the bases themselves through kzg_msm_g2 (host bases): the same bits
    assert np.array_equal(helpers.msm_g2(g2.g2[off:off + n], sc), want)
    # range and length errors
    assert lib.kzg_msm_g2_srs(ctx.handle, g2.handle, (1 << 16) - n + 1, _lib.ptr(sc), n, _lib.ptr(out), C.byref(inf)) == _lib.ERR_POLY_LENGTH
    assert lib.kzg_msm_g2_srs(ctx.handle, g2.handle, 0, None, n, _lib.ptr(out), C.byref(inf)) == _lib.ERR_INVALID_ARG
    small = k.G2SRS.generate(TAU, 8)
    try:
        with pytest.raises(SerializationError):
            k.KZG.new().commit_g2_coeff_form(k.PolynomialCoeffForm(frs_from_ints(list(range(16)))), small)
        with pytest.raises(SrsCapacityExceeded):
            k.KZG.new().commit_g2_eval_form(k.PolynomialEvalForm(frs_from_ints(list(range(16)))), small)
        ev = np.ascontiguousarray(frs_from_ints([1, 2, 3]))
        assert lib.kzg_commit_g2_eval_form(ctx.handle, small.handle, _lib.ptr(ev), 3, _lib.ptr(out), C.byref(inf)) == _lib.ERR_NOT_POWER_OF_TWO
    finally:
        small.close()


def test_an_msm_above_the_per_launch_cap_runs_as_parts():
    """csrc/g2msm_plan.h G2MSM_MAX_LAUNCH = 2^22 pairs: a longer MSM is cut into launches whose sums the host adds.  2^22 + 37 pairs equal the
    sum of the first 2^22 (one launch) and the last 37 (one launch, also against its closed form), added by a two-point MSM."""
    cap = 1 << 22
    n = cap + 37
    ctx = _lib.default_context()
    lib = _lib.load()
    g2 = k.G2SRS.generate(TAU, n)
    try:
        rng = np.random.Generator(np.random.PCG64(11))
        sc = np.ascontiguousarray(rng.integers(0, 1 << 60, size=(n, 4), dtype=np.uint64))       # canonical wire words (< 2^252)
        tail = [random.Random(i).randrange(R_) for i in range(37)]
        sc[cap:] = frs_from_ints(tail)
        inf = C.c_uint8(0)
        whole = np.zeros(16, np.uint64); head = np.zeros(16, np.uint64); last = np.zeros(16, np.uint64)
        assert lib.kzg_msm_g2_srs(ctx.handle, g2.handle, 0, _lib.ptr(sc), n, _lib.ptr(whole), C.byref(inf)) == _lib.OK
        assert lib.kzg_msm_g2_srs(ctx.handle, g2.handle, 0, _lib.ptr(sc), cap, _lib.ptr(head), C.byref(inf)) == _lib.OK
        tail_sc = np.ascontiguousarray(sc[cap:])
        assert lib.kzg_msm_g2_srs(ctx.handle, g2.handle, cap, _lib.ptr(tail_sc), 37, _lib.ptr(last), C.byref(inf)) == _lib.OK
        assert np.array_equal(last, helpers.g2_mul_generator(fr_from_int(horner(tail) * pow(TAU, cap, R_) % R_)))
        assert whole.any() and np.array_equal(whole, helpers.msm_g2(np.stack([head, last]), frs_from_ints([1, 1])))
    finally:
        g2.close()
