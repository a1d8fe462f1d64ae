"""No GPU: the host-checkable half of the encoder's serialized form (`kzg_encode_cosets_batch_bytes`, `kzg_disperse_blobs_bytes`).

  1. `g1_compress_point` / `g1_compress_wire_point` of csrc/g1_decode.h, the way out that the affine conversion behind FK20 takes, built
     for the host with the bound-checked field (tests/hostcheck/g1compresscheck.cpp, g++ -DKZG_BOUND_CHECK) and compared with the host
     encoder `kzg_host::g1_encode_be` and with big integers (tests/coset_bytes_ref.py over pyref): the identity, the generator,
     multiples of the generator with both flags, every point with its negative, and the round trip through `g1_decompress_point`; once
     more under AddressSanitizer and UBSan.
  2. the ABI surface of the two entries: parameter names against the header, the `_lib.py` table, and the error rows that need no device.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pyref
from coset_bytes_ref import IDENTITY_BE, P, compress_be

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
SRC = os.path.join(HERE, "hostcheck", "g1compresscheck.cpp")
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
    m = re.fullmatch(r"g1 compress ok records=(\d+) identity=(\d+) small=(\d+) large=(\d+)", r.stdout.strip())
    assert m, r.stdout[-500:]
    return [int(v) for v in m.groups()]


def record(pt):
    xy = bytes(64) if pt is None else pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")
    return xy + compress_be(pt)


@pytest.fixture(scope="module")
def points():
    """the identity, the generator, its multiples 2 .. 40 and a few large ones, each finite point with its negative"""
    pts = [None]
    scalars = list(range(1, 41)) + [pyref.R_ - 1, pyref.R_ // 2, 0xC0FFEE << 200]
    for s in scalars:
        pt = pyref.ec_mul(s, pyref.G1)
        pts += [pt, pyref.ec_neg(pt)]
    return pts


def test_the_points_cover_what_the_compressor_decides(points):
    assert compress_be(None) == IDENTITY_BE == b"\x40" + bytes(31)
    gen = compress_be(pyref.G1)
    assert gen == bytes([0x80]) + bytes(30) + b"\x01"                                   # y = 2 is the smaller root
    flags = {compress_be(pt)[0] >> 6 for pt in points if pt is not None}
    assert flags == {2, 3}
    for pt in points[1::2]:                                                             # a point and its negative: the flag alone
        a, b = compress_be(pt), compress_be(pyref.ec_neg(pt))
        assert a[1:] == b[1:] and a[0] ^ b[0] == 0x40 and pyref.ec_neg(pt) == (pt[0], P - pt[1])


def test_compressor_against_the_host_encoder_and_big_integers(points, tmp_path):
    exe = str(tmp_path / "g1compresscheck")
    _build(exe, ["-O1"])
    n_finite = len(points) - 1
    records, identity, small, large = _run(exe, [record(pt) for pt in points], tmp_path)
    assert (records, identity) == (len(points), 1)
    assert small == large == n_finite // 2                                              # every pair (P, -P) has one of each


def test_compressor_stand_alone_under_asan_ubsan(points, tmp_path):
    exe = str(tmp_path / "g1compresscheck_san")
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    recs = [record(pt) for pt in points[:21]]
    assert _run(exe, recs, tmp_path, env)[0] == len(recs)


# ---- the ABI surface (the library loads without a GPU) -------------------------------------------------------------------------------------
ENTRIES = {
    "kzg_encode_cosets_batch_bytes": ["ctx", "srs", "blobs_be", "count", "poly_len", "eval_form", "n", "chunk_len", "out_commitments_be", "out_ys_be",
                                      "out_proofs_be", "bad_index"],
    "kzg_disperse_blobs_bytes": ["ctx", "srs", "g2_srs", "g2_trailing", "trailing_first_power", "srs_order", "blobs_be", "count", "poly_len", "n", "chunk_len",
                                 "claimed_len", "out_commitments_be", "out_length_commitments_be", "out_length_proofs_be", "out_ys_be", "out_proofs_be", "bad_index"],
}


def test_the_c_abi_declares_the_two_entries_with_these_parameters():
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read(), flags=re.S)
    from rust_kzg_bn254_amd import _lib
    lib = _lib.load()
    for name, params in ENTRIES.items():
        decl = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert decl, name
        names = [re.sub(r"\[.*\]", "", p).split()[-1].lstrip("*") for p in decl.group(1).split(",")]
        assert names == params, (name, names)
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == len(params) and hasattr(lib, name)
    import rust_kzg_bn254_amd as k
    assert callable(k.KZG.encode_cosets_batch_bytes) and callable(k.KZG.disperse_blobs_bytes)


def test_the_error_rows_that_need_no_device():
    from rust_kzg_bn254_amd import _lib as L
    lib = L.load()
    z = (C.c_uint8 * 64)()
    bad = C.c_uint64(7)
    # row 1: null handles, whatever else is wrong (no handle is dereferenced)
    assert lib.kzg_encode_cosets_batch_bytes(None, None, z, 1, 16, 0, 32, 1, z, z, z, C.byref(bad)) == L.ERR_INVALID_ARG
    assert lib.kzg_encode_cosets_batch_bytes(None, None, None, 0, 3, 0, 5, 3, None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.kzg_disperse_blobs_bytes(None, None, None, None, 0, 16, z, 1, 16, 32, 1, 16, z, z, z, z, z, C.byref(bad)) == L.ERR_INVALID_ARG
    assert lib.kzg_disperse_blobs_bytes(None, None, None, None, 0, 15, None, 0, 16, 32, 1, 12, None, None, None, None, None, None) == L.ERR_INVALID_ARG
    assert bad.value == 7
    # the Python surface refuses shapes before it looks for a device
    import rust_kzg_bn254_amd as k

    class FakeSrs:
        handle = None

        def __len__(self):
            return 16

    kz = k.KZG.__new__(k.KZG)
    blob = bytes(16 * 32)
    with pytest.raises(k.errors.InvalidInputLength):
        kz.encode_cosets_batch_bytes(blob[:-1], FakeSrs(), 32)
    with pytest.raises(k.errors.GenericError, match="one length"):
        kz.encode_cosets_batch_bytes([blob, blob[:32]], FakeSrs(), 32)
    with pytest.raises(k.errors.FFTError):
        kz.encode_cosets_batch_bytes(blob, FakeSrs(), 48)
    with pytest.raises(k.errors.GenericError, match="chunk length"):
        kz.encode_cosets_batch_bytes(blob, FakeSrs(), 32, chunk_len=16)
    with pytest.raises(k.errors.SrsCapacityExceeded):
        kz.encode_cosets_batch_bytes(np.zeros((2, 32 * 32), np.uint8), FakeSrs(), 64)
    with pytest.raises(k.errors.GenericError, match="commitments, values"):
        kz.encode_cosets_batch_bytes(blob, FakeSrs(), 32, commitments=False, values=False, proofs=False)
    with pytest.raises(k.errors.GenericError, match="uint8"):
        kz.disperse_blobs_bytes(np.zeros((2, 16, 4), np.uint64), FakeSrs(), None, None, 64, 16, 32)
