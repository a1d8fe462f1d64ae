"""CPU: the host-only entries of the G2 feature.  `kzg_g2_decompress_be` against the Python decoder it can replace
(`helpers.read_g2_powers_of_2`) on the reference's g2.point.powerOf2, its errors with the index of the first bad point, the same decoder
and the G2 MSM planner as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (a subprocess: nothing is loaded into
Python under a sanitizer), and `kzg_verify_length_proof` on a header built from a small known polynomial and tau with the fixed-base G2
multiplication of the C-ABI and big-integer G1 arithmetic."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyref
import rust_kzg_bn254_amd as k
from pyref import R_
from rust_kzg_bn254_amd import _lib, helpers, verifier
from rust_kzg_bn254_amd.errors import DeserializationError, NotOnCurveError
from rust_kzg_bn254_amd.fr import fr_from_int

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
G2_FILE = os.path.join(HERE, "golden", "g2.point.powerOf2")


def _decode(data):
    n = len(data) // 64
    out = np.zeros((max(n, 1), 16), np.uint64)
    bad = C.c_uint64(2 ** 64 - 1)
    buf = np.frombuffer(data, dtype=np.uint8)
    rc = _lib.load().kzg_g2_decompress_be(buf.ctypes.data_as(_lib.u8p), n, _lib.ptr(out), C.byref(bad))
    return rc, bad.value, out[:n]


def test_decoder_equals_the_python_decoder_bit_for_bit():
    data = open(G2_FILE, "rb").read()
    rc, _, got = _decode(data)
    assert rc == _lib.OK
    want = helpers.read_g2_powers_of_2(G2_FILE)
    assert got.shape == want.shape == (28, 16) and np.array_equal(got, want)
    assert np.array_equal(k.G2SRS.decompress(data), want)


def test_decoder_errors_carry_the_first_bad_index(tmp_path):
    data = bytearray(open(G2_FILE, "rb").read())

    def damaged(i, fn):
        d = bytearray(data)
        fn(d, 64 * i)
        return bytes(d)

    def flag0(d, o): d[o] &= 0x3F                       # noqa: E704
    def flag1(d, o): d[o] = (d[o] & 0x3F) | 0x40        # noqa: E704
    def big_c0(d, o): d[o + 32:o + 64] = b"\xff" * 32   # noqa: E704
    def big_c1(d, o): d[o:o + 32] = bytes([d[o] | 0x3F]) + b"\xff" * 31   # noqa: E704
    for i, fn in ((0, flag0), (5, flag1), (27, big_c0), (13, big_c1)):
        rc, bad, _ = _decode(damaged(i, fn))
        assert (rc, bad) == (_lib.ERR_DESERIALIZE, i), fn.__name__
        with pytest.raises(DeserializationError):
            k.G2SRS.decompress(damaged(i, fn))
        p = tmp_path / "damaged"
        p.write_bytes(damaged(i, fn))
        with pytest.raises(DeserializationError):       # the Python decoder raises the same class
            helpers.read_g2_powers_of_2(str(p))
    # an x with no point on the twist (about every second x), found by stepping the last byte of point 3; the Python decoder agrees on which
    for t in range(1, 40):
        d = bytearray(data)
        d[64 * 3 + 63] = (d[64 * 3 + 63] + t) % 256
        rc, bad, _ = _decode(bytes(d))
        p = tmp_path / "off"
        p.write_bytes(bytes(d))
        if rc == _lib.OK:
            helpers.read_g2_powers_of_2(str(p))
            continue
        assert (rc, bad) == (_lib.ERR_NOT_ON_CURVE, 3)
        with pytest.raises(NotOnCurveError):
            helpers.read_g2_powers_of_2(str(p))
        break
    else:
        raise AssertionError("no off-curve x among 39 neighbours")
    # two bad points: the first one is reported
    d = bytearray(damaged(20, flag0))
    d[64 * 7] &= 0x3F
    assert _decode(bytes(d))[:2] == (_lib.ERR_DESERIALIZE, 7)
    assert _decode(b"")[0] == _lib.OK


def test_decoder_and_planner_stand_alone_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "g2_sanitize_main")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                           "-I" + CSRC, "-I" + os.path.join(HERE, "hostcheck"), os.path.join(HERE, "hostcheck", "g2_sanitize_main.cpp"), "-lpthread", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, G2_FILE], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "g2 sanitize ok 28", (r.stdout[-500:], r.stderr[-3000:])


def _header(f, tau, N, d):
    """(C, C2, pi2, [tau^(N-d)]_1) of the coefficients f by closed forms: [f(tau)]_1, [f(tau)]_2, [tau^(N-d) f(tau)]_2"""
    ft = sum(c * pow(tau, i, R_) for i, c in enumerate(f)) % R_
    sh = pow(tau, N - d, R_)
    g1 = (1, 2)
    return (pyref.point_to_wire(pyref.ec_mul(ft, g1)).reshape(8), helpers.g2_mul_generator(fr_from_int(ft)),
            helpers.g2_mul_generator(fr_from_int(ft * sh % R_)), pyref.point_to_wire(pyref.ec_mul(sh, g1)).reshape(8))


def test_verify_length_proof_accepts_and_rejects():
    tau, N = 0x1234567890ABCDEF1234567, 64
    f = [3, 1, 4, 1, 5, 9, 2, 6]                                            # degree 7
    C_, C2, pi2, shift = _header(f, tau, N, 8)
    assert verifier.verify_length_proof(C_, C2, pi2, shift)
    assert verifier.verify_length_proof(*_header(f, tau, N, 16))            # a larger claimed length is honest too
    assert verifier.verify_length_proof(*_header(f, tau, N, 64))            # d = N: the shift is G1 itself
    # each element altered (to another valid group element)
    other1 = pyref.point_to_wire(pyref.ec_mul(77, (1, 2))).reshape(8)
    other2 = helpers.g2_mul_generator(fr_from_int(78))
    assert not verifier.verify_length_proof(other1, C2, pi2, shift)
    assert not verifier.verify_length_proof(C_, other2, pi2, shift)
    assert not verifier.verify_length_proof(C_, C2, other2, shift)
    assert not verifier.verify_length_proof(C_, C2, pi2, other1)
    # a claimed length below deg f + 1: the only proof the prover can form without tau^N and beyond is the one for ITS length, presented with the
    # verifier's shift [tau^(N-4)]_1 for d = 4
    _, _, _, shift4 = _header(f, tau, N, 4)
    assert not verifier.verify_length_proof(C_, C2, pi2, shift4)
    # off-curve inputs are errors, not "false"
    bad1 = C_.copy(); bad1[0] ^= np.uint64(1)
    bad2 = C2.copy(); bad2[0] ^= np.uint64(1)
    with pytest.raises(NotOnCurveError):
        verifier.verify_length_proof(bad1, C2, pi2, shift)
    with pytest.raises(NotOnCurveError):
        verifier.verify_length_proof(C_, C2, pi2, bad1)
    with pytest.raises(NotOnCurveError):
        verifier.verify_length_proof(C_, bad2, pi2, shift)
    with pytest.raises(NotOnCurveError):
        verifier.verify_length_proof(C_, C2, bad2, shift)
    ok = _lib.i32(0)
    assert _lib.load().kzg_verify_length_proof(None, _lib.ptr(C2), _lib.ptr(pi2), _lib.ptr(shift), C.byref(ok)) == _lib.ERR_INVALID_ARG
    # the zero polynomial: all three elements are the identity
    z8, z16 = np.zeros(8, np.uint64), np.zeros(16, np.uint64)
    assert verifier.verify_length_proof(z8, z16, z16, shift)
