"""Host-only (no GPU, no library): csrc/host_fiat_shamir.h built by g++ with a serial parallel-for (tests/hostcheck/fscheck.cpp), each
piece of the Fiat-Shamir codec against a twin written here with hashlib and big integers: digest -> Fr at the modulus, the compressed
G1 encoding, and both random-linear-combination transcripts on either side of their job sizes (64 rows; 1024 / l items)."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import pyref
from pyref import P, R_

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rust-kzg-bn254_amd", "csrc")
u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def fs(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fscheck") / "libfscheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, os.path.join(HERE, "hostcheck", "fscheck.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.fs_digest_to_fr_wire.argtypes = [u8p, u64p]
    lib.fs_fr_wire_to_be_bytes.argtypes = [u64p, u8p]
    lib.fs_g1_serialize_compressed_ark.argtypes = [u64p, u8p]
    lib.fs_blob_padded_len.argtypes = [C.c_size_t]
    lib.fs_blob_padded_len.restype = C.c_size_t
    lib.fs_powers_of.argtypes = [u64p, C.c_size_t, u64p]
    lib.fs_r_powers.argtypes = [u64p] * 5 + [C.c_size_t, u64p]
    lib.fs_multiproof_r_powers.argtypes = [u64p, C.c_size_t, u64p, u64p, u64p, u64p, C.c_size_t, C.c_size_t, C.c_size_t, u64p]
    return lib


def p64(a):
    return a.ctypes.data_as(u64p)


def words(arrs, width):
    return np.ascontiguousarray(np.stack(arrs), dtype=np.uint64).reshape(len(arrs), width)


def compressed_py(pt):
    """ark-serialize compressed G1Affine: x little-endian, 0x80 = y is the larger root, 0x40 = infinity"""
    if pt is None:
        return bytes(31) + b"\x40"
    b = bytearray(pt[0].to_bytes(32, "little"))
    if pt[1] > (P - 1) // 2:
        b[31] |= 0x80
    return bytes(b)


def powers_py(data, n):
    r = int.from_bytes(hashlib.sha256(data).digest(), "big") % R_
    return [pow(r, i, R_) for i in range(n)]


def random_points(rnd, count):
    """`count` points as (affine or None) with both signs of y and the identity among them"""
    pts = [pyref.ec_mul(rnd.randrange(1, R_), (1, 2)) for _ in range(3)]
    pts += [(pts[0][0], P - pts[0][1]), None]
    return [pts[rnd.randrange(len(pts))] for _ in range(count)]


def wire(pt):
    return np.zeros(8, np.uint64) if pt is None else pyref.point_to_wire(pt)


@pytest.mark.parametrize("value", [0, 1, R_ - 1, R_, R_ + 1, 2 * R_, (1 << 256) - 1], ids=["0", "1", "r-1", "r", "r+1", "2r", "ones"])
def test_digest_to_fr_wire_at_the_modulus(fs, value):
    dig = np.frombuffer(value.to_bytes(32, "big"), np.uint8).copy()
    out = np.zeros(4, np.uint64)
    fs.fs_digest_to_fr_wire(dig.ctypes.data_as(u8p), p64(out))
    assert pyref.from_limbs(out) < R_                                         # a reduced Montgomery residue ...
    assert pyref.fr_from_mont(out) == value % R_                              # ... of the digest as a big-endian integer mod r
    back = np.zeros(32, np.uint8)
    fs.fs_fr_wire_to_be_bytes(p64(out), back.ctypes.data_as(u8p))
    assert back.tobytes() == (value % R_).to_bytes(32, "big")


def test_g1_serialize_compressed_ark_identity_generator_and_larger_root(fs):
    rnd = random.Random(7)
    cases = [None, (1, 2)]
    while len(cases) < 4:                                                     # one point with the larger y root, and its negative (the smaller)
        pt = pyref.ec_mul(rnd.randrange(1, R_), (1, 2))
        if pt[1] > (P - 1) // 2:
            cases += [pt, (pt[0], P - pt[1])]
    flags = []
    for pt in cases:
        out = np.zeros(32, np.uint8)
        w = wire(pt)
        fs.fs_g1_serialize_compressed_ark(p64(w), out.ctypes.data_as(u8p))
        assert out.tobytes() == compressed_py(pt), pt
        flags.append(int(out[31]) & 0xC0)
    assert flags == [0x40, 0x00, 0x80, 0x00]                                  # (the generator's y = 2 is the smaller root)


@pytest.mark.parametrize("length", [0, 1, 32, 33, 64, 65, 32 * 1000, 32 * 1024 + 1])
def test_blob_padded_len(fs, length):
    assert fs.fs_blob_padded_len(length) == pyref.next_pow2(-(-length // 32))


@pytest.mark.parametrize("n", [1, 2, 65])
def test_r_powers_host_against_hashlib(fs, n):
    """batch.rs:76-168: domain tag (24 B) || 8 zero bytes || u64be(n) || n x u64be(len) || n x (C | z | y | proof); 65 rows = two jobs of the fan-out"""
    rnd = random.Random(n)
    cs, ps = random_points(rnd, n), random_points(rnd, n)
    z_int = [rnd.randrange(R_) for _ in range(n)]
    y_int = [rnd.randrange(R_) for _ in range(n)]
    z_int[0], y_int[-1] = 0, R_ - 1
    lens = [1 << rnd.randrange(0, 13) for _ in range(n)]
    c_w, p_w = words([wire(c) for c in cs], 8), words([wire(p) for p in ps], 8)
    z_w, y_w = pyref.frs_to_mont(z_int), pyref.frs_to_mont(y_int)
    l_w = np.array(lens, np.uint64)
    out = np.zeros((n, 4), np.uint64)
    fs.fs_r_powers(p64(c_w), p64(z_w), p64(y_w), p64(p_w), p64(l_w), n, p64(out))
    data = b"EIGENDA_RCKZGBATCH___V1_" + bytes(8) + n.to_bytes(8, "big") + b"".join(v.to_bytes(8, "big") for v in lens)
    for i in range(n):
        data += compressed_py(cs[i]) + z_int[i].to_bytes(32, "big") + y_int[i].to_bytes(32, "big") + compressed_py(ps[i])
    assert len(data) == 40 + 8 * n + 128 * n
    want = powers_py(data, n)
    assert pyref.frs_from_mont(out) == want
    r_w = pyref.fr_to_mont(want[1] if n > 1 else 5)                           # powers_of alone, from 1
    again = np.zeros((n, 4), np.uint64)
    fs.fs_powers_of(p64(r_w), n, p64(again))
    assert pyref.frs_from_mont(again) == [pow(want[1] if n > 1 else 5, i, R_) for i in range(n)]


@pytest.mark.parametrize("count,l", [(1, 1), (3, 4), (1025, 1)])
def test_multiproof_r_powers_host_against_hashlib(fs, count, l):
    """header || commitments || one digest per item (tag || row || coset || l values || proof); 1025 items of l = 1 = two jobs of the fan-out"""
    rnd = random.Random(100 * count + l)
    n, M = 64, 3
    cs, ps = random_points(rnd, M), random_points(rnd, count)
    rows = [rnd.randrange(M) for _ in range(count)]
    ks = [rnd.randrange(n // l) for _ in range(count)]
    y_int = [[rnd.randrange(R_) for _ in range(l)] for _ in range(count)]
    y_int[0][0], y_int[-1][l - 1] = 0, R_ - 1
    c_w, p_w = words([wire(c) for c in cs], 8), words([wire(p) for p in ps], 8)
    y_w = np.ascontiguousarray(np.stack([pyref.frs_to_mont(v) for v in y_int]))
    out = np.zeros((count, 4), np.uint64)
    fs.fs_multiproof_r_powers(p64(c_w), M, p64(np.array(rows, np.uint64)), p64(np.array(ks, np.uint64)), p64(y_w), p64(p_w), count, n, l, p64(out))
    data = b"KZGBN254_COSETBATCH__V1_" + n.to_bytes(8, "big") + l.to_bytes(8, "big") + M.to_bytes(8, "big") + count.to_bytes(8, "big")
    data += b"".join(compressed_py(c) for c in cs)
    for i in range(count):
        item = b"KZGBN254_COSETITEM___V1_" + rows[i].to_bytes(8, "big") + ks[i].to_bytes(8, "big")
        item += b"".join(v.to_bytes(32, "big") for v in y_int[i]) + compressed_py(ps[i])
        data += hashlib.sha256(item).digest()
    assert pyref.frs_from_mont(out) == powers_py(data, count)
