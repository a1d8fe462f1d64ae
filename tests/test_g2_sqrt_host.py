"""CPU check of the device decoder of gnark-compressed G2 points (rust-kzg-bn254_amd/csrc/g2_decode.h): the byte decode, the square
root in Fq by a windowed fixed-exponent chain, the square root in Fq2 with two exponentiations (direct and swapped branch, a1 = 0),
the sign rule and the decoder of one point.

tests/hostcheck/g2sqrtcheck.cpp compiles the header with g++ and -DKZG_BOUND_CHECK, so that every lazy-reduction bound the formulas
rely on is an abort(), and compares every result BY VALUE with the independent Fq / Fq2 of csrc/host_pairing.h and the host decoder of
csrc/host_g2_decode.h.  It is a stand-alone program: it runs once as it is and once under AddressSanitizer +
UndefinedBehaviorSanitizer (a subprocess; nothing is loaded into Python under a sanitizer).
"""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
SRC = os.path.join(HERE, "hostcheck", "g2sqrtcheck.cpp")
G2_FILE = os.path.join(HERE, "golden", "g2.point.powerOf2")


def _build(exe, extra):
    subprocess.check_call(["g++", "-std=c++17", "-DKZG_BOUND_CHECK", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", *extra, "-I" + CSRC, SRC, "-o", exe])


def _run(exe, env=None):
    r = subprocess.run([exe, G2_FILE], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "KZG_BOUND_CHECK" not in r.stderr, r.stderr[-3000:]
    m = re.fullmatch(r"g2 sqrt ok direct=(\d+) swapped=(\d+) none=(\d+) points=(\d+)", r.stdout.strip())
    assert m, r.stdout[-500:]
    return [int(v) for v in m.groups()]


def test_decoder_math_by_value_with_every_bound_checked(tmp_path):
    exe = str(tmp_path / "g2sqrtcheck")
    _build(exe, ["-O1"])
    direct, swapped, none, points = _run(exe)
    # every branch of the square root is taken often: about a quarter, a quarter and a half of random elements
    assert direct >= 100 and swapped >= 100 and none >= 100 and direct + swapped + none >= 2000
    assert points == 28


def test_decoder_math_stand_alone_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "g2sqrtcheck_san")
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    assert _run(exe, env)[3] == 28


def test_the_c_abi_declares_the_device_decoder():
    header = open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read()
    from rust_kzg_bn254_amd import _lib
    for name in ("kzg_g2_decompress_be_device", "kzg_g2srs_load_compressed_be"):
        assert re.search(r"\b%s\(" % name, header) and name in _lib.PROTOTYPES
    assert "#define KZG_G2_CHECK_SUBGROUP   1u" in header and "#define KZG_G2_REJECT_GENERATOR 2u" in header
    assert (_lib.G2_CHECK_SUBGROUP, _lib.G2_REJECT_GENERATOR) == (1, 2)
