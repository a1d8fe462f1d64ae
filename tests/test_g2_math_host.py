"""CPU check of the device G2 math headers (rust-kzg-bn254_amd/csrc/fq2.h, curve_g2.h).

tests/hostcheck/g2check.cpp compiles them with g++ and -DKZG_BOUND_CHECK, so that every lazy-reduction bound the formulas rely on is
an abort(), and compares every result BY VALUE with the independent Fq2 / G2 arithmetic of csrc/host_pairing.h (other limb size, other
coordinates).  Every entry of the library returns 0 on agreement.
"""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import fe_operands as fo
from pyref import P, R_

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostcheck", "g2check.cpp")
SO = os.path.join(HERE, "hostcheck", "libg2check.so")
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")

u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
u8p = C.POINTER(C.c_uint8)
i32p = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def g2c():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("field29.h", "fq2.h", "curve_g2.h", "curve.h", "fe_invert.h", "host_pairing.h", "host_curve.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DKZG_BOUND_CHECK", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-I" + CSRC, "-o", SO, SRC])
    return C.CDLL(SO)


def _point(g2c, k):
    out = np.zeros(16, np.uint64)
    kw = np.array([(k >> (64 * j)) & (2 ** 64 - 1) for j in range(4)], np.uint64)
    g2c.g2c_mul_generator(kw.ctypes.data_as(u64p), out.ctypes.data_as(u64p))
    return out


@pytest.fixture(scope="module")
def points(g2c):
    """1 200 random multiples of the generator, wire form, and their scalars"""
    rnd = random.Random(2)
    ks = [rnd.randrange(1, R_) for _ in range(1200)]
    return ks, np.stack([_point(g2c, k) for k in ks])


def _neg(p):
    """-p of a wire point: (x, m - y) per component, in the Montgomery form (negation commutes with the radix)"""
    q = p.copy()
    if not q.any():
        return q
    for c in (2, 3):
        v = sum(int(q[4 * c + j]) << (64 * j) for j in range(4))
        v = (P - v) % P
        for j in range(4):
            q[4 * c + j] = (v >> (64 * j)) & (2 ** 64 - 1)
    return q


def _w32(pts):
    return np.ascontiguousarray(pts, dtype=np.uint64).view(np.uint32).reshape(-1).copy()


def test_generator_constant(g2c):
    assert g2c.g2c_generator_matches() == 0


def test_products_and_squares_on_extreme_limbs(g2c):
    """fq2_mul / fq2_mul_lazy / fq2_sqr / fq2_mul_fq on the extreme SIGNED limb patterns of fe_operands (limbs at +-(2^29 - 1), alternating
    signs, one hot limb, zero) and on the lazy value ranges the group law feeds them, in BOTH components"""
    rnd = random.Random(31)
    pats = fo.extreme_patterns(rnd)
    lazy3 = [fo.unnormalise(fo.limbs(v), rnd) for v in fo.lazy_values(P, rnd, 12) if abs(v) < 3 * P]          # 4 * 3 * 3 = 36 m^2
    lazy6 = [fo.unnormalise(fo.limbs(v), rnd) for v in fo.lazy_values(P, rnd, 12) if abs(v) < 6 * P]          # squares: (6 + 6)^2 = 144 m^2
    arr = lambda a, b: (C.c_int32 * 18)(*(list(a) + list(b)))       # noqa: E731
    ops = pats + lazy3
    n = 0
    for i in range(len(ops)):
        for step in (1, 7, 13):
            a = arr(ops[i], ops[(i * 3 + step) % len(ops)])
            b = arr(ops[(i * 5 + step + 1) % len(ops)], ops[(i * 11 + step + 2) % len(ops)])
            for op in (0, 2, 3):
                assert g2c.g2c_product_vs_host(a, b, op) == 0, (i, step, op)
            n += 1
    sq = pats + lazy6
    for i in range(len(sq)):
        for step in (0, 1, 5):                                      # step 0: equal components (a0 - a1 == 0)
            a = arr(sq[i], sq[(i + step) % len(sq)])
            assert g2c.g2c_product_vs_host(a, a, 1) == 0, (i, step)
    assert n > 300


def test_inverse(g2c):
    rnd = random.Random(32)
    vals = [(0, 0), (1, 0), (0, 1), (P - 1, P - 1), (1, P - 1), (0, 5)] + [(rnd.randrange(P), rnd.randrange(P)) for _ in range(100)]
    for c0, c1 in vals:
        w = np.array([((v << 256) % P >> (32 * j)) & 0xFFFFFFFF for v in (c0, c1) for j in range(8)], np.uint32)
        assert g2c.g2c_inverse_vs_host(w.ctypes.data_as(u32p)) == 0, (c0, c1)


def _chain(g2c, pts, signs, inline_slow=0):
    wire = _w32(pts) if len(pts) else np.zeros(1, np.uint32)
    sg = np.array(list(signs) + [0], dtype=np.uint8)
    return g2c.g2c_madd_chain_vs_host(wire.ctypes.data_as(u32p), sg.ctypes.data_as(u8p), C.c_size_t(len(pts)), inline_slow)


def test_madd_chains(g2c, points):
    _, pts = points
    rnd = random.Random(33)
    signs = [rnd.randrange(2) for _ in range(len(pts))]
    assert _chain(g2c, pts, signs) == 0                             # 1 200 random points: the stored form holds at every step
    assert _chain(g2c, pts[:300], signs[:300], inline_slow=1) == 0
    a, b = pts[5], pts[9]
    z = np.zeros(16, np.uint64)
    cases = [([a, a], [0, 0]), ([a, a, a, b], [0, 0, 0, 1]), ([a, a], [0, 1]), ([a, a, b], [0, 1, 0]), ([a, _neg(a)], [0, 0]),
             ([a, _neg(a), a], [0, 0, 0]), ([z, a, z], [0, 0, 1]), ([z, z], [0, 0]), ([], []), ([a] * 17, [0] * 17), ([a] * 17, [1] * 17),
             ([a, b, a, b, _neg(a), _neg(b)], [0, 0, 1, 1, 1, 1])]
    for pts_, sg in cases:
        for inl in (0, 1):
            assert _chain(g2c, np.stack(pts_) if pts_ else [], sg, inl) == 0, (len(pts_), sg)


def test_sum_equals_scalar_sum(g2c, points):
    """the chain of [k_i] G2 is [sum k_i] G2: ties the device formulas to the fixed-base multiplication as well"""
    ks, pts = points
    total = _point(g2c, sum(ks[:64]) % R_)
    chain = np.concatenate([pts[:64], _neg(total)[None, :]])
    # sum - [sum k] G2 == identity: the chain's last addition is P + (-P)
    assert _chain(g2c, chain, [0] * 65) == 0
    wire = _w32(chain)
    sg = np.zeros(66, np.uint8)
    assert g2c.g2c_add_halves_vs_host(wire.ctypes.data_as(u32p), sg.ctypes.data_as(u8p), C.c_size_t(65), 0) == 0


def test_full_add_doubling_and_memory_format(g2c, points):
    _, pts = points
    rnd = random.Random(34)
    for n in (2, 3, 10, 64, 65, 200):
        sel = np.stack([pts[rnd.randrange(len(pts))] for _ in range(n)])
        signs = np.array([rnd.randrange(2) for _ in range(n)], np.uint8)
        wire = _w32(sel)
        for dbl in (0, 1, 5):
            assert g2c.g2c_add_halves_vs_host(wire.ctypes.data_as(u32p), signs.ctypes.data_as(u8p), C.c_size_t(n), dbl) == 0, (n, dbl)
    a = pts[77]
    # a + a and a + (-a) through the full add of STORED values, an empty half on either side, both empty
    z = np.zeros(16, np.uint64)
    for pair, sg in (([a, a], [0, 0]), ([a, a], [0, 1]), ([z, a], [0, 0]), ([a, z], [0, 0]), ([z, z], [0, 0])):
        wire = _w32(np.stack(pair)); s = np.array(sg, np.uint8)
        for dbl in (0, 2):
            assert g2c.g2c_add_halves_vs_host(wire.ctypes.data_as(u32p), s.ctypes.data_as(u8p), C.c_size_t(2), dbl) == 0, (sg, dbl)


def test_exceptional_cases_in_every_operand_position(g2c, points):
    _, pts = points
    a, b = pts[3], pts[4]
    z = np.zeros(16, np.uint64)
    pairs = [(a, b), (a, a), (a, _neg(a)), (_neg(a), a), (z, a), (a, z), (z, z)]
    for x, y in pairs:
        for which in (0, 1, 2):
            assert g2c.g2c_pair_vs_host(_w32(x).ctypes.data_as(u32p), _w32(y).ctypes.data_as(u32p), which) == 0, which


def test_wire_round_trip_and_twist_check(g2c, points):
    _, pts = points
    for p in list(pts[:40]) + [np.zeros(16, np.uint64)]:
        assert g2c.g2c_wire_roundtrip(_w32(p).ctypes.data_as(u32p)) == 0
    off = pts[0].copy()
    off[0] ^= np.uint64(1)                                          # x.c0 changed: off the twist on both sides
    assert g2c.g2c_wire_roundtrip(_w32(off).ctypes.data_as(u32p)) == 0
    off = pts[1].copy(); off[12] ^= np.uint64(2)
    assert g2c.g2c_wire_roundtrip(_w32(off).ctypes.data_as(u32p)) == 0
