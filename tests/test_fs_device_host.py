"""Host-only (no GPU, no library): csrc/dev_sha256.h and csrc/coset_item_stream.h -- the code the hashing kernels of csrc/fsdevice.hip run
one lane per message -- compiled by g++ (tests/hostcheck/fsdevcheck.cpp).  Digests at the padding boundaries against hashlib; the item
message of the coset transcript, block by block as a lane produces it, against the item bytes of
`verifier.compute_multiproof_r_powers_py` (the identity proof, a point and its negative so that both sign flags appear, values 0, 1 and
r - 1) and, through the digests, against that function's weights; the non-canonical flag.  The same file with its own main() runs once
under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program (nothing is loaded into Python under a sanitizer)."""
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
SRC = os.path.join(HERE, "hostcheck", "fsdevcheck.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-I" + CSRC]
u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
ROW_LENS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 2120]


@pytest.fixture(scope="module")
def fsdev(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fsdevcheck") / "libfsdevcheck.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", *FLAGS, SRC, "-o", so])
    lib = C.CDLL(so)
    lib.fsdev_sha256.argtypes = [u8p, C.c_size_t, u8p]
    lib.fsdev_item_blocks.argtypes = [C.c_size_t]
    lib.fsdev_on_device.argtypes = [C.c_int, C.c_size_t, C.c_size_t]
    lib.fsdev_item_blocks.restype = C.c_size_t
    lib.fsdev_item.argtypes = [u64p, u64p, C.c_uint64, C.c_uint64, C.c_size_t, u8p, u8p]
    lib.fsdev_item.restype = C.c_uint32
    return lib


@pytest.fixture(scope="module")
def V():
    from rust_kzg_bn254_amd import verifier
    return verifier


def u8(a):
    return a.ctypes.data_as(u8p)


def p64(a):
    return a.ctypes.data_as(u64p)


@pytest.mark.parametrize("length", ROW_LENS)
def test_sha256_block_function_and_tail_against_hashlib(fsdev, length):
    """55 / 56: the length still fits the block of the 0x80 byte / no longer; 63 / 64 / 65 and 119 / 120 / 128: the same one block on"""
    msg = np.frombuffer(random.Random(length).randbytes(length), np.uint8).copy() if length else np.zeros(0, np.uint8)
    out = np.zeros(32, np.uint8)
    fsdev.fsdev_sha256(u8(msg), length, u8(out))
    assert out.tobytes() == hashlib.sha256(msg.tobytes()).digest()


def special_points():
    """wire points: the identity, a point whose y is the larger root, its negative"""
    rnd = random.Random(11)
    while True:
        pt = pyref.ec_mul(rnd.randrange(1, R_), (1, 2))
        if pt[1] > (P - 1) // 2:
            return [np.zeros(8, np.uint64), pyref.point_to_wire(pt), pyref.point_to_wire((pt[0], P - pt[1]))]


def item(V, fsdev, ys_w, proof_w, c, k):
    l = len(ys_w)
    stream = np.zeros(64 * fsdev.fsdev_item_blocks(l), np.uint8)
    dig = np.zeros(32, np.uint8)
    bad = fsdev.fsdev_item(p64(ys_w), p64(proof_w), c, k, l, u8(stream), u8(dig))
    return stream.tobytes(), dig.tobytes(), bad


@pytest.mark.parametrize("l", [1, 2, 16, 64])
def test_item_stream_is_the_item_bytes_of_the_python_transcript(fsdev, V, l):
    from rust_kzg_bn254_amd import helpers
    from rust_kzg_bn254_amd.fr import fr_to_int
    rnd = random.Random(l)
    points = special_points()
    n, count = 4096, len(points)
    y_int = [[rnd.randrange(R_) for _ in range(l)] for _ in range(count)]
    y_int[0][0], y_int[1][0], y_int[2][l - 1] = 0, 1, R_ - 1
    ys = np.ascontiguousarray(np.stack([pyref.frs_to_mont(v) for v in y_int]))
    rows, ks = [0, 2, 1], [rnd.randrange(n // l) for _ in range(count)]
    flags, digests = [], []
    for i in range(count):
        stream, dig, bad = item(V, fsdev, ys[i], points[i], rows[i], ks[i])
        want = V.COSET_ITEM_DOMAIN + rows[i].to_bytes(8, "big") + ks[i].to_bytes(8, "big")
        want += b"".join(fr_to_int(ys[i, j]).to_bytes(32, "big") for j in range(l)) + helpers.serialize_compressed(points[i])
        assert len(want) == 72 + 32 * l and bad == 0
        assert stream[:len(want)] == want
        tail = stream[len(want):]                                             # 0x80, zeros, the bit length: to a multiple of 64 bytes
        assert len(stream) % 64 == 0 and 9 <= len(tail) < 73
        assert tail == b"\x80" + bytes(len(tail) - 9) + (8 * len(want)).to_bytes(8, "big")
        assert dig == hashlib.sha256(want).digest()
        flags.append(want[-1] & 0xC0)
        digests.append(dig)
    assert flags == [0x40, 0x80, 0x00]
    # ... and through the digests, the weights of the Python transcript
    commitments = [points[1], points[0], points[2]]
    head = V.COSET_BATCH_DOMAIN + b"".join(v.to_bytes(8, "big") for v in (n, l, len(commitments), count))
    head += b"".join(helpers.serialize_compressed(c) for c in commitments)
    r = helpers.hash_to_field_element(head + b"".join(digests))
    assert np.array_equal(helpers.compute_powers(r, count), V.compute_multiproof_r_powers_py(commitments, rows, ks, ys, points, n))


def test_non_canonical_inputs_raise_the_flag(fsdev, V):
    """a value >= r, a coordinate >= p: the kernel reports them and the caller takes the host transcript"""
    ident = np.zeros(8, np.uint64)
    ok = pyref.frs_to_mont([5])
    assert item(V, fsdev, ok, ident, 0, 0)[2] == 0
    for value in (R_, R_ + 1, (1 << 256) - 1):
        bad_y = np.array([[(value >> (64 * j)) & (2**64 - 1) for j in range(4)]], np.uint64)
        assert item(V, fsdev, bad_y, ident, 0, 0)[2] == 1
    assert item(V, fsdev, np.array([[(R_ - 1 >> (64 * j)) & (2**64 - 1) for j in range(4)]], np.uint64), ident, 0, 0)[2] == 0
    for pos in (0, 4):
        pt = pyref.point_to_wire((1, 2)).copy()
        pt[pos:pos + 4] = [(P >> (64 * j)) & (2**64 - 1) for j in range(4)]
        assert item(V, fsdev, ok, pt, 0, 0)[2] == 1


def test_automatic_mode_takes_the_device_only_inside_the_measured_envelope(fsdev):
    """measured to win (profiles/fs_device.md): N >= 4 096, l <= 64, >= 2 MiB of values.  Few long items -- the shape a lane per stream does not
    fit -- and small batches stay on the host whatever their bytes; the forced modes ignore the shape"""
    on = lambda count, l, mode=0: bool(fsdev.fsdev_on_device(mode, count, l))  # noqa: E731
    assert [on(*s) for s in ((65536, 1), (4096, 16), (4096, 64), (65536, 16), (65536, 64), (1 << 20, 1))] == [True] * 6
    assert [on(*s) for s in ((256, 1), (4096, 1), (256, 16), (256, 64), (4095, 64), (4096, 8))] == [False] * 6      # below the count or the bytes
    assert [on(*s) for s in ((256, 256), (64, 1024), (1, 65536), (4096, 128), (65536, 128), (1 << 16, 4096))] == [False] * 6    # long items
    assert on(1, 1 << 20, mode=2) and on(1, 1, mode=2) and not on(65536, 64, mode=1)


def test_stand_alone_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "fsdevcheck_san")
    subprocess.check_call(["g++", "-O1", "-g", "-DFSDEVCHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           *FLAGS, SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "fsdevcheck ok", (r.stdout[-500:], r.stderr[-3000:])
