"""Host-only (no GPU): coset items in their serialized form.

1-3. The strict device decoder of gnark-compressed G1 points (rust-kzg-bn254_amd/csrc/g1_decode.h), the scalar decoder beside it and the
     second producer of csrc/coset_item_stream.h, built for the host with the bound-checked field (tests/hostcheck/g1decodecheck.cpp,
     -DKZG_BOUND_CHECK: every lazy-reduction bound is an abort()) and fed records whose expectations are big integers computed here
     (tests/coset_bytes_ref.py) or taken from tests/golden/srs.g1.points.string.  A stand-alone program: it runs once as it is and once under
     AddressSanitizer + UndefinedBehaviorSanitizer, as a subprocess; nothing is loaded into Python under a sanitizer.
4.   kzg_coset_items_encode_be against big integers.
5.   kzg_compute_multiproof_r_powers_bytes equals kzg_compute_multiproof_r_powers, bit for bit, on the encoded form of the same items, and
     verifier.py's pure-Python transcript.
"""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import pyref
from coset_bytes_ref import (IDENTITY_BE, KIND_DESERIALIZE, KIND_IDENTITY, KIND_NOT_ON_CURVE, KIND_OK, P, R_, compress_be, decode_be, record, values_be,
                             x_without_point)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
SRC = os.path.join(HERE, "hostcheck", "g1decodecheck.cpp")
G1_FILE = os.path.join(HERE, "golden", "g1.point")
u8p = C.POINTER(C.c_uint8)


def _build(exe, extra):
    subprocess.check_call(["g++", "-std=c++17", "-DKZG_BOUND_CHECK", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", *extra, "-I" + CSRC, SRC, "-o", exe])


def _run(exe, records, tmp_path, env=None):
    path = str(tmp_path / "records.bin")
    with open(path, "wb") as f:
        f.write(b"".join(records))
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "KZG_BOUND_CHECK" not in r.stderr, r.stderr[-3000:]
    m = re.fullmatch(r"g1 decode ok records=(\d+) finite=(\d+) identity=(\d+) deserialize=(\d+) not_on_curve=(\d+)", r.stdout.strip())
    assert m, r.stdout[-500:]
    return [int(v) for v in m.groups()]


@pytest.fixture(scope="module")
def golden_bytes():
    data = open(G1_FILE, "rb").read()
    assert len(data) == 3000 * 32
    return [data[32 * i:32 * i + 32] for i in range(3000)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("g1decodecheck") / "g1decodecheck")
    _build(path, ["-O1"])
    return path


def golden_records(golden_bytes, points, step=1):
    """the file's points against srs.g1.points.string, then P and -P compressed by the big-integer encoder"""
    recs = []
    for i in range(0, len(golden_bytes), step):
        x, y = points[i]
        recs.append(golden_bytes[i] + bytes([KIND_OK]) + x.to_bytes(32, "big") + y.to_bytes(32, "big"))
        for pt in ((x, y), (x, P - y)):
            recs.append(compress_be(pt) + bytes([KIND_OK]) + pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big"))
    return recs


def refusal_cases(golden_bytes):
    """(bytes, expected kind) of every refusal the decoder documents, and the one encoding of the identity"""
    g = golden_bytes[17]
    cases = [(IDENTITY_BE, KIND_IDENTITY)]
    for pos in (1, 16, 31):
        b = bytearray(IDENTITY_BE); b[pos] = 1
        cases.append((bytes(b), KIND_DESERIALIZE))
    b = bytearray(IDENTITY_BE); b[0] = 0x41
    cases.append((bytes(b), KIND_DESERIALIZE))
    cases.append((bytes([g[0] & 0x3F]) + g[1:], KIND_DESERIALIZE))                      # flag 0b00 on a golden x
    cases.append((bytes(32), KIND_DESERIALIZE))                                         # flag 0b00, x = 0
    for x in (P, P + 1, (1 << 254) - 1):
        for flag in (0x80, 0xC0):
            b = bytearray(x.to_bytes(32, "big")); b[0] |= flag
            cases.append((bytes(b), KIND_DESERIALIZE))
    x0 = int.from_bytes(bytes([g[0] & 0x3F]) + g[1:], "big")
    x_off = x_without_point(x0 + 1)
    for flag in (0x80, 0xC0):
        b = bytearray(x_off.to_bytes(32, "big")); b[0] |= flag
        cases.append((bytes(b), KIND_NOT_ON_CURVE))
    b = bytearray((P - 1).to_bytes(32, "big")); b[0] |= 0x80                           # the largest canonical x: whatever it is, by the twin
    cases.append((bytes(b), decode_be(bytes(b))[0]))
    return cases


def test_decoder_on_the_golden_points_with_every_bound_checked(exe, golden_bytes, test_srs_points, tmp_path):
    for i in (0, 1, 1499, 2999):                                                        # the twin agrees with the golden strings
        assert decode_be(golden_bytes[i]) == (KIND_OK, test_srs_points[i])
    recs = golden_records(golden_bytes, test_srs_points)
    records, finite, identity, deser, off = _run(exe, recs, tmp_path)
    assert (records, finite, identity, deser, off) == (9000, 9000, 0, 0, 0)


def test_decoder_refusals_each_with_its_kind(exe, golden_bytes, tmp_path):
    cases = refusal_cases(golden_bytes)
    for b, kind in cases:
        assert decode_be(b)[0] == kind, (b.hex(), kind)                                 # the twin gives the documented kind ...
    recs = [record(b) for b, _ in cases] + golden_records(golden_bytes[:8], [decode_be(b)[1] for b in golden_bytes[:8]])
    kinds = [k for _, k in cases]
    got = _run(exe, recs, tmp_path)                                                     # ... and the decoder gives the twin's
    assert got == [len(recs), kinds.count(KIND_OK) + 24, kinds.count(KIND_IDENTITY), kinds.count(KIND_DESERIALIZE), kinds.count(KIND_NOT_ON_CURVE)]
    assert kinds.count(KIND_IDENTITY) == 1 and kinds.count(KIND_DESERIALIZE) >= 12 and kinds.count(KIND_NOT_ON_CURVE) >= 2


def test_decoder_stand_alone_under_asan_ubsan(golden_bytes, test_srs_points, tmp_path):
    exe = str(tmp_path / "g1decodecheck_san")
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    recs = golden_records(golden_bytes, test_srs_points, step=25) + [record(b) for b, _ in refusal_cases(golden_bytes)]
    assert _run(exe, recs, tmp_path, env)[0] == len(recs)


# ---- the library's host entries (no GPU: the library loads without one) -----------------------------------------------------------------
@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    return k


def some_points(rnd):
    pts = [pyref.ec_mul(rnd.randrange(1, R_), (1, 2)) for _ in range(3)]
    return pts + [(pts[0][0], P - pts[0][1])]


def make_items(rnd, count, l):
    """values (0, 1 and r - 1 among them) and proofs (one the identity) as integers / affine points"""
    base = some_points(rnd)
    vals = [[rnd.randrange(R_) for _ in range(l)] for _ in range(count)]
    edge = [0, 1, R_ - 1]
    for j, v in enumerate(edge):
        vals[(j // l) % count][j % l] = v
    proofs = [base[rnd.randrange(len(base))] for _ in range(count)]
    proofs[count // 2] = None
    return vals, proofs


@pytest.mark.parametrize("l", [1, 16])
@pytest.mark.parametrize("count", [1, 5])
def test_encode_against_big_integers(k, count, l):
    rnd = random.Random(1000 * count + l)
    vals, proofs = make_items(rnd, count, l)
    ys = np.stack([pyref.frs_to_mont(row) for row in vals])
    ys_be, proofs_be = k.verifier.encode_coset_items(ys, pyref.points_to_wire(proofs))
    assert ys_be == b"".join(values_be(row) for row in vals)
    assert proofs_be == b"".join(compress_be(pt) for pt in proofs)
    assert proofs_be[32 * (count // 2):32 * (count // 2) + 32] == IDENTITY_BE
    assert k.helpers.compress_g1_be(pyref.points_to_wire(proofs)) == proofs_be
    # values only / proofs only
    assert k.verifier.encode_coset_items(ys, None) == (ys_be, None)
    assert k.verifier.encode_coset_items(None, pyref.points_to_wire(proofs)) == (None, proofs_be)


def test_encode_refuses_words_that_are_not_below_the_modulus(k):
    lib = k.load()
    ys = pyref.to_limbs(R_).reshape(1, 4).copy()                                        # the wire words of "r": not a residue
    out = np.zeros(32, np.uint8)
    assert lib.kzg_coset_items_encode_be(k._lib.ptr(ys), None, 1, 1, out.ctypes.data_as(u8p), None) == k._lib.ERR_INVALID_ARG
    pt = np.zeros(8, np.uint64); pt[:4] = pyref.to_limbs(P); pt[4] = 1
    assert lib.kzg_coset_items_encode_be(None, k._lib.ptr(pt), 1, 1, None, out.ctypes.data_as(u8p)) == k._lib.ERR_INVALID_ARG
    # a pair is NULL together; chunk_len = 0 with values
    assert lib.kzg_coset_items_encode_be(k._lib.ptr(ys), None, 1, 1, None, None) == k._lib.ERR_INVALID_ARG
    assert lib.kzg_coset_items_encode_be(k._lib.ptr(ys), None, 1, 0, out.ctypes.data_as(u8p), None) == k._lib.ERR_INVALID_ARG
    assert lib.kzg_coset_items_encode_be(None, None, 0, 1, None, None) == k._lib.OK


@pytest.mark.parametrize("l", [1, 16])
@pytest.mark.parametrize("count", [1, 3, 300])
def test_r_powers_from_bytes_equal_r_powers_from_words(k, count, l):
    rnd = random.Random(77 * count + l)
    vals, proofs = make_items(rnd, count, l)
    commitments = some_points(rnd)[:2]
    ci = [rnd.randrange(2) for _ in range(count)]
    ki = [rnd.randrange(4096 // l) for _ in range(count)]
    ys = np.stack([pyref.frs_to_mont(row) for row in vals])
    pf, cm = pyref.points_to_wire(proofs), pyref.points_to_wire(commitments)
    ys_be, proofs_be = k.verifier.encode_coset_items(ys, pf)
    cm_be = k.helpers.compress_g1_be(cm)
    want = k.verifier.compute_multiproof_r_powers(list(cm), ci, ki, ys, list(pf), 4096)
    got = k.verifier.compute_multiproof_r_powers_bytes(cm_be, ci, ki, ys_be, proofs_be, 4096, l)
    assert got.shape == (count, 4) and np.array_equal(got, want)
    assert np.array_equal(np.asarray(k.verifier.compute_multiproof_r_powers_py(list(cm), ci, ki, ys, list(pf), 4096), np.uint64).reshape(-1, 4), want)
    # a different byte anywhere is a different transcript
    flipped = bytearray(ys_be); flipped[-1] ^= 1
    assert not np.array_equal(k.verifier.compute_multiproof_r_powers_bytes(cm_be, ci, ki, bytes(flipped), proofs_be, 4096, l)[1:], want[1:]) or count == 1


def test_the_c_abi_declares_the_bytes_entries():
    header = open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read()
    from rust_kzg_bn254_amd import _lib
    for name in ("kzg_g1_decompress_be_device", "kzg_coset_items_decode_be", "kzg_coset_items_encode_be", "kzg_compute_multiproof_r_powers_bytes",
                 "kzg_verify_multiproof_batch_bytes"):
        assert re.search(r"\b%s\(" % name, header) and name in _lib.PROTOTYPES
