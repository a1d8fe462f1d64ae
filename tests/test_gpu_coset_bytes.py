"""-m gpu: coset items in their serialized form on the device -- `kzg_g1_decompress_be_device`, `kzg_coset_items_decode_be` and the fused
verifier `kzg_verify_multiproof_batch_bytes` (csrc/g1_decode.h, csrc/cosetbytes.hip, the second producer of csrc/coset_item_stream.h).
Golden points bit-equal, the smallest bad index whatever the launch geometry, encode -> decode round trips, the fused verifier against the
decoded entry (verdict and weights, host and device transcript), rejections, the error table and the bound-checked build.  Everything
that must ACCEPT uses a known-tau SRS of 4 096 points, as tests/test_gpu_multiproof_verify.py does."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pyref
from coset_bytes_ref import IDENTITY_BE, P, R_, compress_be, x_without_point

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TAU = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/coset-bytes/v1").digest(), "big") % R_
N_DOMAIN = 4096
u8p = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


class World:
    """Three random polynomials of 4 096 evaluations on a known-tau SRS; per chunk length their proofs and cosets, decoded and serialized."""

    def __init__(self, k):
        self.k, self.n = k, N_DOMAIN
        self.srs = k.SRS.generate(TAU, self.n)
        self.kz = k.KZG.new()
        self.kz.calculate_and_store_roots_of_unity(self.n * 32)
        rnd = random.Random(4242)
        self.polys = [k.PolynomialEvalForm(pyref.frs_to_mont([rnd.randrange(R_) for _ in range(self.n)])) for _ in range(3)]
        self.commitments = [self.kz.commit_eval_form(p, self.srs) for p in self.polys]
        self.commitments_be = k.helpers.compress_g1_be(np.stack(self.commitments))
        self._by_l = {}

    def at(self, l):
        if l not in self._by_l:
            proofs = [self.kz.compute_multiproofs(p, self.srs, l) for p in self.polys]
            cosets = [self.kz.cosets(p, l) for p in self.polys]
            g2 = self.k.helpers.g2_mul_generator(self.k.fr.fr_from_int(pow(TAU, l, R_)))
            self._by_l[l] = (proofs, cosets, g2)
        return self._by_l[l]

    def items(self, l, count, seed=0):
        """`count` items over the three commitments (repeated when count exceeds the 3 n / l the world has): decoded and serialized"""
        proofs, cosets, g2 = self.at(l)
        m = self.n // l
        rnd = random.Random(1000 * l + count + seed)
        rows = [rnd.randrange(3) for _ in range(count)]
        ks = [rnd.randrange(m) for _ in range(count)]
        ks[0] = m - 1
        ys = np.ascontiguousarray(np.stack([cosets[c][kk] for c, kk in zip(rows, ks)]))
        pf = np.ascontiguousarray(np.stack([proofs[c][kk] for c, kk in zip(rows, ks)]))
        ys_be, pf_be = self.k.verifier.encode_coset_items(ys, pf)
        return rows, ks, ys, pf, ys_be, pf_be, g2


@pytest.fixture(scope="module")
def world(k):
    return World(k)


@pytest.fixture(scope="module")
def golden(golden_dir, test_srs_wire):
    data = open(os.path.join(golden_dir, "g1.point"), "rb").read()
    assert len(data) == 3000 * 32
    return data, test_srs_wire


def raw_decompress(k, data, n, sentinel=0xA5):
    """the C entry itself: (rc, bad index, out, inf), the outputs prefilled so that "not written" shows"""
    L = k._lib
    buf = np.frombuffer(data, np.uint8)
    out = np.full((max(n, 1), 8), 0xA5A5A5A5A5A5A5A5, np.uint64)
    inf = np.full(max(n, 1), sentinel, np.uint8)
    bad = C.c_uint64(1 << 40)
    rc = L.load().kzg_g1_decompress_be_device(L.default_context().handle, buf.ctypes.data_as(u8p), n, L.ptr(out), inf.ctypes.data_as(u8p), C.byref(bad))
    return rc, bad.value, out, inf


# ---- 1. kzg_g1_decompress_be_device on the golden points -----------------------------------------------------------------------------
def test_golden_points_decode_bit_equal(k, golden):
    data, wire = golden
    out, inf = k.helpers.decompress_g1_device(data, return_is_infinity=True)
    assert out.shape == (3000, 8) and np.array_equal(out, wire) and not inf.any()
    assert k.helpers.decompress_g1_device(b"").shape == (0, 8)
    assert k.helpers.compress_g1_be(out) == data                                        # ... and the host encoder gives the file back


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_block_boundaries_with_an_identity_at_either_end(k, golden, n):
    data, wire = golden
    for where in (0, n - 1):
        b = bytearray(data[:32 * n])
        b[32 * where:32 * where + 32] = IDENTITY_BE
        out, inf = k.helpers.decompress_g1_device(bytes(b), return_is_infinity=True)
        want = wire[:n].copy()
        want[where] = 0
        assert np.array_equal(out, want)
        assert inf.tolist() == [i == where for i in range(n)]


# ---- 2. the smallest bad index ---------------------------------------------------------------------------------------------------------
def damage(b32, how):
    x = int.from_bytes(bytes([b32[0] & 0x3F]) + b32[1:], "big")
    if how == "flag":                                                                   # 0b00: deserialize
        return bytes([b32[0] & 0x3F]) + b32[1:]
    if how == "x=p":                                                                    # not canonical: deserialize
        b = bytearray(P.to_bytes(32, "big")); b[0] |= b32[0] & 0xC0
        return bytes(b)
    b = bytearray(x_without_point(x + 1).to_bytes(32, "big")); b[0] |= b32[0] & 0xC0    # "off": no point of that x
    return bytes(b)


@pytest.mark.parametrize("kinds", [("flag", "off", "x=p"), ("off", "x=p", "flag"), ("x=p", "flag", "off")])
def test_smallest_bad_index_wins_with_its_own_kind(k, golden, kinds):
    data, _ = golden
    L = k._lib
    b = bytearray(data)
    for idx, how in zip((7, 256, 2999), kinds):
        b[32 * idx:32 * idx + 32] = damage(data[32 * idx:32 * idx + 32], how)
    want = L.ERR_NOT_ON_CURVE if kinds[0] == "off" else L.ERR_DESERIALIZE
    rc, bad, out, inf = raw_decompress(k, bytes(b), 3000)
    assert (rc, bad) == (want, 7)
    assert (out == 0xA5A5A5A5A5A5A5A5).all() and (inf == 0xA5).all()                    # on error the outputs are not written
    exc = k.errors.NotOnCurveError if kinds[0] == "off" else k.errors.DeserializationError
    with pytest.raises(exc, match=r"point 7\b"):
        k.helpers.decompress_g1_device(bytes(b))
    # without the damage at 7, the next one reports itself
    b[32 * 7:32 * 7 + 32] = data[32 * 7:32 * 7 + 32]
    rc, bad, _, _ = raw_decompress(k, bytes(b), 3000)
    assert (rc, bad) == (L.ERR_NOT_ON_CURVE if kinds[1] == "off" else L.ERR_DESERIALIZE, 256)
    # argument checks, then the context still decodes
    lib, h = L.load(), L.default_context().handle
    buf = np.frombuffer(data, np.uint8)
    out8 = np.zeros((1, 8), np.uint64)
    assert lib.kzg_g1_decompress_be_device(None, buf.ctypes.data_as(u8p), 1, L.ptr(out8), None, None) == L.ERR_INVALID_ARG
    assert lib.kzg_g1_decompress_be_device(h, None, 1, L.ptr(out8), None, None) == L.ERR_INVALID_ARG
    assert lib.kzg_g1_decompress_be_device(h, buf.ctypes.data_as(u8p), 1, None, None, None) == L.ERR_INVALID_ARG
    assert lib.kzg_g1_decompress_be_device(h, buf.ctypes.data_as(u8p), (1 << 28) + 1, L.ptr(out8), None, None) == L.ERR_TOO_LARGE
    assert lib.kzg_g1_decompress_be_device(h, None, 0, None, None, None) == L.OK
    assert lib.kzg_g1_decompress_be_device(h, buf.ctypes.data_as(u8p), 1, L.ptr(out8), None, None) == L.OK     # out_is_infinity and bad_index may be NULL


# ---- 3. encode -> decode round trip -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l,count", [(1, 257), (16, 3), (64, 257)])
def test_encode_decode_round_trip(k, l, count):
    rnd = random.Random(31 * l + count)
    vals = [[rnd.randrange(R_) for _ in range(l)] for _ in range(count)]
    vals[0][0], vals[count - 1][l - 1], vals[count // 2][0] = 0, R_ - 1, 1              # r - 1 is accepted
    base = [pyref.ec_mul(rnd.randrange(1, R_), (1, 2)) for _ in range(3)]
    base += [(base[0][0], P - base[0][1]), None]
    pts = [base[rnd.randrange(len(base))] for _ in range(count)]
    pts[count - 1] = None
    ys, pf = np.stack([pyref.frs_to_mont(row) for row in vals]), pyref.points_to_wire(pts)
    ys_be, pf_be = k.verifier.encode_coset_items(ys, pf)
    ys2, pf2 = k.verifier.decode_coset_items(ys_be, pf_be, l)
    assert ys2.shape == (count, l, 4) and np.array_equal(ys2, ys) and np.array_equal(pf2, pf)
    only_y, none_p = k.verifier.decode_coset_items(ys_be, None, l)                      # recovery decodes values only
    assert none_p is None and np.array_equal(only_y, ys)
    none_y, only_p = k.verifier.decode_coset_items(None, pf_be, l)
    assert none_y is None and np.array_equal(only_p, pf)
    if count > 200:
        bad = bytearray(ys_be)
        pos = 32 * (200 * l + l - 1)
        bad[pos:pos + 32] = R_.to_bytes(32, "big")                                      # a value equal to r, the last of item 200
        L = k._lib
        yb, pb = np.frombuffer(bytes(bad), np.uint8), np.frombuffer(pf_be, np.uint8)
        oy, op = np.full((count, l, 4), 7, np.uint64), np.full((count, 8), 7, np.uint64)
        idx, arr = C.c_uint64(0), L.i32(-1)
        rc = L.load().kzg_coset_items_decode_be(L.default_context().handle, yb.ctypes.data_as(u8p), pb.ctypes.data_as(u8p), count, l, L.ptr(oy), L.ptr(op),
                                                C.byref(idx), C.byref(arr))
        assert (rc, idx.value, arr.value) == (L.ERR_DESERIALIZE, 200, 2)
        assert (oy == 7).all() and (op == 7).all()
        with pytest.raises(k.errors.DeserializationError, match=r"value of item 200\b"):
            k.verifier.decode_coset_items(bytes(bad), pf_be, l)
        badp = bytearray(pf_be)
        badp[32 * 5] &= 0x3F                                                            # a bad proof is reported before a bad value
        with pytest.raises(k.errors.DeserializationError, match=r"proof 5\b"):
            k.verifier.decode_coset_items(bytes(bad), bytes(badp), l)


# ---- 3b. more than one staged piece, more than one launch --------------------------------------------------------------------------------
# The bytes go up in pieces of 32 768 points or values through two pinned halves (csrc/byte_stager.h) and a kernel starts behind every
# 131 072.  A pool of POOL distinct items is tiled up to the count: POOL is odd, so it divides neither a piece nor a launch, and a copy or
# launch offset that is wrong by a whole piece reads other bytes.  The yardstick is the pool's own decode by the same entry (compared with
# the golden points and the host conversion here), tiled the same way.
POOL = 1021


def tiled(pool_bytes, n):
    return bytearray((pool_bytes * (n // POOL + 1))[:32 * n])


@pytest.fixture(scope="module")
def point_pool(k, golden):
    data, wire = golden
    out = k.helpers.decompress_g1_device(data[:32 * POOL])
    assert np.array_equal(out, wire[:POOL])
    return data[:32 * POOL], out


@pytest.fixture(scope="module")
def value_pool(k):
    rnd = random.Random(1021)
    vals = [0, R_ - 1] + [rnd.randrange(R_) for _ in range(POOL - 2)]
    data = b"".join(v.to_bytes(32, "big") for v in vals)
    out, _ = k.verifier.decode_coset_items(data, None, 1)
    assert np.array_equal(out[:, 0], pyref.frs_to_mont(vals))
    return data, out


def test_points_across_three_pieces_are_bit_equal(k, point_pool):
    data, out = point_pool
    n = 65537
    b = tiled(data, n)
    b[:32] = b[32 * (n - 1):] = IDENTITY_BE
    got, inf = k.helpers.decompress_g1_device(bytes(b), return_is_infinity=True)
    want = out[np.arange(n) % POOL]
    want[0] = want[n - 1] = 0
    assert np.array_equal(got, want)
    assert inf[0] and inf[n - 1] and inf.sum() == 2


def test_bad_points_in_the_second_launch(k, point_pool):
    data, _ = point_pool
    L = k._lib
    n = 131074
    b = tiled(data, n)
    b[32 * 131072:32 * 131073] = damage(bytes(b[32 * 131072:32 * 131073]), "off")
    b[32 * 131073:32 * 131074] = damage(bytes(b[32 * 131073:32 * 131074]), "x=p")
    rc, bad, _, _ = raw_decompress(k, bytes(b), n)
    assert (rc, bad) == (L.ERR_NOT_ON_CURVE, 131072)


def test_values_across_a_second_launch(k, value_pool):
    data, out = value_pool
    L = k._lib
    n = 131074
    b = tiled(data, n)
    got, _ = k.verifier.decode_coset_items(bytes(b), None, 1)
    assert np.array_equal(got, out[np.arange(n) % POOL])
    b[32 * 131072:32 * 131073] = R_.to_bytes(32, "big")
    b[32 * 131073:32 * 131074] = b"\xff" * 32
    yb = np.frombuffer(bytes(b), np.uint8)
    oy = np.zeros((n, 1, 4), np.uint64)
    idx, arr = C.c_uint64(0), L.i32(-1)
    rc = L.load().kzg_coset_items_decode_be(L.default_context().handle, yb.ctypes.data_as(u8p), None, n, 1, L.ptr(oy), None, C.byref(idx), C.byref(arr))
    assert (rc, idx.value, arr.value) == (L.ERR_DESERIALIZE, 131072, 2)


def test_one_stager_serves_proofs_and_values_with_three_pieces_each(k, point_pool, value_pool):
    n = 65537
    ys, pf = k.verifier.decode_coset_items(bytes(tiled(value_pool[0], n)), bytes(tiled(point_pool[0], n)), 1)
    assert np.array_equal(ys, value_pool[1][np.arange(n) % POOL]) and np.array_equal(pf, point_pool[1][np.arange(n) % POOL])


# ---- 4. the fused verifier ----------------------------------------------------------------------------------------------------------------
def check_fused_equals_decoded(k, world, l, count):
    V = k.verifier
    rows, ks, ys, pf, ys_be, pf_be, g2 = world.items(l, count)
    ctx = world.srs.ctx
    want_rp = V.compute_multiproof_r_powers(world.commitments, rows, ks, ys, list(pf), world.n)
    assert V.verify_multiproof_batch(world.commitments, rows, ks, ys, list(pf), world.n, world.srs, g2)
    for mode in (0, 2, 1):                                                              # automatic, device transcript from bytes, host
        ctx.set_transcript_device(mode)
        try:
            ok, rp = V.verify_multiproof_batch_bytes(world.commitments_be, rows, ks, ys_be, pf_be, world.n, l, world.srs, g2, return_r_powers=True)
        finally:
            ctx.set_transcript_device(0)
        assert ok and np.array_equal(rp, want_rp), (l, count, mode)
    # supplied weights: used as they are, and returned
    mine = pyref.frs_to_mont([random.Random(l * count + i).randrange(R_) for i in range(count)])
    ok, rp = V.verify_multiproof_batch_bytes(world.commitments_be, rows, ks, ys_be, pf_be, world.n, l, world.srs, g2, r_powers=mine, return_r_powers=True)
    assert ok and np.array_equal(rp, mine)
    assert V.verify_multiproof_batch(world.commitments, rows, ks, ys, list(pf), world.n, world.srs, g2, r_powers=mine)
    return rows, ks, ys, pf, ys_be, pf_be, g2


@pytest.mark.parametrize("l", [1, 16, 64])
@pytest.mark.parametrize("count", [1, 3, 257])
def test_fused_verifier_accepts_with_the_decoded_entrys_weights(k, world, l, count):
    check_fused_equals_decoded(k, world, l, count)


def test_fused_verifier_inside_the_automatic_envelope(k, world):
    """count = 4 096, l = 16: 2 MiB of values, the automatic mode takes the device transcript (csrc/host_fiat_shamir.h)"""
    check_fused_equals_decoded(k, world, 16, 4096)


def test_fused_verifier_with_an_identity_commitment_and_proof(k, world):
    """the zero polynomial: commitment, values and proofs are the identity / zero; 0x40 || zeros all the way through"""
    V = k.verifier
    l, count = 16, 3
    rows, ks, ys, pf, _, _, g2 = world.items(l, count)
    zero_c = np.zeros(8, np.uint64)
    cms = list(world.commitments) + [zero_c]
    rows = [3, rows[1], rows[2]]
    ys = ys.copy(); ys[0] = 0
    pf = pf.copy(); pf[0] = 0
    ys_be, pf_be = V.encode_coset_items(ys, pf)
    cm_be = k.helpers.compress_g1_be(np.stack(cms))
    assert cm_be[96:128] == IDENTITY_BE and pf_be[:32] == IDENTITY_BE
    assert V.verify_multiproof_batch(cms, rows, ks, ys, list(pf), world.n, world.srs, g2)
    ok, rp = V.verify_multiproof_batch_bytes(cm_be, rows, ks, ys_be, pf_be, world.n, l, world.srs, g2, return_r_powers=True)
    assert ok and np.array_equal(rp, V.compute_multiproof_r_powers(cms, rows, ks, ys, list(pf), world.n))
    assert V.verify_multiproof_batch_bytes(cm_be, [], [], b"", b"", world.n, l, world.srs, g2) is True       # count = 0


# ---- 5. rejections ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", [1, 16])
def test_rejections_agree_with_the_decoded_entry(k, world, l):
    V = k.verifier
    count = 37
    rows, ks, ys, pf, ys_be, pf_be, g2 = world.items(l, count, seed=5)

    def both(ys_be_, pf_be_):
        ys_, pf_ = V.decode_coset_items(ys_be_, pf_be_, l)
        decoded = V.verify_multiproof_batch(world.commitments, rows, ks, ys_, list(pf_), world.n, world.srs, g2)
        fused = V.verify_multiproof_batch_bytes(world.commitments_be, rows, ks, ys_be_, pf_be_, world.n, l, world.srs, g2)
        assert fused == decoded
        return fused

    assert both(ys_be, pf_be) is True
    flipped = bytearray(ys_be); flipped[32 * (11 * l) + 31] ^= 1                        # one value byte (the value stays below r)
    assert both(bytes(flipped), pf_be) is False
    j = next(j for j in range(1, count) if pf_be[32 * j:32 * j + 32] != pf_be[:32])
    swapped = bytearray(pf_be); swapped[:32] = pf_be[32 * j:32 * j + 32]                # another valid proof
    assert both(ys_be, bytes(swapped)) is False
    sign = bytearray(pf_be); sign[32 * 9] ^= 0x40                                       # 0b10 <-> 0b11: the negated proof
    assert both(ys_be, bytes(sign)) is False


# ---- 6. the error table -------------------------------------------------------------------------------------------------------------------
def test_error_table_in_the_documented_order_then_an_accepting_call(k, world, test_srs_wire):
    L = k._lib
    lib = L.load()
    ctx = world.srs.ctx
    n, l, count = world.n, 16, 4
    m = n // l
    rows, ks, ys, pf, ys_be, pf_be, g2 = world.items(l, count, seed=9)
    cm = np.frombuffer(world.commitments_be, np.uint8)
    yb, pb = np.frombuffer(ys_be, np.uint8), np.frombuffer(pf_be, np.uint8)
    ci, ki = np.array(rows, np.uint64), np.array(ks, np.uint64)
    ok, idx, arr = L.i32(7), C.c_uint64(99), L.i32(-1)
    small_srs = k.SRS(test_srs_wire[:8], order=8)
    lag = world.srs.lagrange(64)

    def call(ctx_h=ctx.handle, srs_h=world.srs.handle, cm_=cm, M=3, ci_=ci, ki_=ki, ys_=yb, pf_=pb, count_=count, n_=n, l_=l, g2_=g2, ok_=C.byref(ok)):
        B = lambda a: None if a is None else a.ctypes.data_as(u8p)             # noqa: E731
        W = lambda a: None if a is None else L.ptr(a)                          # noqa: E731
        idx.value, arr.value = 99, -1
        return lib.kzg_verify_multiproof_batch_bytes(ctx_h, srs_h, B(cm_), M, W(ci_), W(ki_), B(ys_), B(pf_), count_, n_, l_, None, W(g2_), ok_, None,
                                                     C.byref(idx), C.byref(arr))

    assert call() == L.OK and ok.value == 1
    ok.value = 7
    # 1. the checks of kzg_verify_multiproof_batch, in its order
    for kw in (dict(ctx_h=None), dict(srs_h=None), dict(ok_=None), dict(cm_=None), dict(ci_=None), dict(ki_=None), dict(ys_=None), dict(pf_=None),
               dict(g2_=None), dict(srs_h=lag.handle)):
        assert call(**kw) == L.ERR_INVALID_ARG, kw
    assert call(n_=0) == L.ERR_NOT_POWER_OF_TWO and call(n_=96) == L.ERR_NOT_POWER_OF_TWO
    assert call(n_=1 << 25) == L.ERR_DOMAIN
    for kw in (dict(n_=1, l_=1), dict(l_=3), dict(l_=0), dict(l_=n)):
        assert call(**kw) == L.ERR_INVALID_ARG, kw
    assert call(srs_h=small_srs.handle) == L.ERR_SRS_CAPACITY_EXCEEDED
    assert call(ki_=np.array([5, 6, 7, m], np.uint64)) == L.ERR_INVALID_ARG
    assert call(M=max(rows)) == L.ERR_INVALID_ARG
    huge = np.zeros((1 << 28) // l + 1, np.uint64)
    assert call(ci_=huge, ki_=huge, count_=len(huge)) == L.ERR_TOO_LARGE
    del huge
    # 2.-5. the bytes, one array at a time and together
    bad_c = cm.copy(); bad_c[32 * 1] &= 0x3F                                            # commitment 1: flag 0b00
    bad_p = pb.copy()
    off = bytearray(x_without_point(int.from_bytes(bytes([pf_be[64] & 0x3F]) + pf_be[65:96], "big") + 1).to_bytes(32, "big")); off[0] |= 0x80
    bad_p[64:96] = np.frombuffer(bytes(off), np.uint8)                                  # proof 2: no point of that x
    bad_y = yb.copy(); bad_y[32 * (3 * l + 5):32 * (3 * l + 5) + 32] = 0xFF             # item 3, value 5: above r
    bad_g2 = g2.copy(); bad_g2[0] ^= 1
    assert (call(cm_=bad_c), idx.value, arr.value) == (L.ERR_DESERIALIZE, 1, 0)
    assert (call(pf_=bad_p), idx.value, arr.value) == (L.ERR_NOT_ON_CURVE, 2, 1)
    assert (call(ys_=bad_y), idx.value, arr.value) == (L.ERR_DESERIALIZE, 3, 2)
    assert call(g2_=bad_g2) == L.ERR_G2_TAU_NOT_ON_CURVE
    assert (call(cm_=bad_c, pf_=bad_p, ys_=bad_y, g2_=bad_g2), idx.value, arr.value) == (L.ERR_DESERIALIZE, 1, 0)       # the commitment first
    assert (call(pf_=bad_p, ys_=bad_y, g2_=bad_g2), idx.value, arr.value) == (L.ERR_NOT_ON_CURVE, 2, 1)
    assert (call(ys_=bad_y, g2_=bad_g2), idx.value, arr.value) == (L.ERR_DESERIALIZE, 3, 2)
    assert call(ki_=np.array([5, 6, 7, m], np.uint64), cm_=bad_c) == L.ERR_INVALID_ARG                                  # the index checks before the bytes
    assert ok.value == 7                                                                # no error path writes the verdict
    # the Python surface names the array and the index
    V = k.verifier
    with pytest.raises(k.errors.DeserializationError, match=r"commitment 1\b"):
        V.verify_multiproof_batch_bytes(bad_c.tobytes(), rows, ks, ys_be, pf_be, n, l, world.srs, g2)
    with pytest.raises(k.errors.NotOnCurveError, match=r"proof 2\b"):
        V.verify_multiproof_batch_bytes(world.commitments_be, rows, ks, ys_be, bad_p.tobytes(), n, l, world.srs, g2)
    with pytest.raises(k.errors.DeserializationError, match=r"value of item 3\b"):
        V.verify_multiproof_batch_bytes(world.commitments_be, rows, ks, bad_y.tobytes(), pf_be, n, l, world.srs, g2)
    with pytest.raises(k.errors.NotOnCurveError, match="G2_TAU not on curve"):
        V.verify_multiproof_batch_bytes(world.commitments_be, rows, ks, ys_be, pf_be, n, l, world.srs, bad_g2)
    # then one accepting call on the same context
    assert call() == L.OK and ok.value == 1
    assert V.verify_multiproof_batch(world.commitments, rows, ks, ys, list(pf), n, world.srs, g2)
    lag.close(); small_srs.close()


# ---- 7. one small case of every new kernel under the bound-checked build ---------------------------------------------------------------
def test_small_case_of_every_new_kernel(k, world, golden):
    """k_g1_decode_be<wire>, k_fr_decode_be, k_g1_decode_be<device format> and k_coset_item_digests_bytes, each once (the workload of the
    bound-checked child below; cheap enough to run here as well)"""
    data, wire = golden
    assert np.array_equal(k.helpers.decompress_g1_device(data[:32 * 257]), wire[:257])
    rows, ks, ys, pf, ys_be, pf_be, g2 = world.items(16, 3)
    ys2, pf2 = k.verifier.decode_coset_items(ys_be, pf_be, 16)
    assert np.array_equal(ys2, ys) and np.array_equal(pf2, pf)
    ctx = world.srs.ctx
    ctx.set_transcript_device(2)
    try:
        assert k.verifier.verify_multiproof_batch_bytes(world.commitments_be, rows, ks, ys_be, pf_be, world.n, 16, world.srs, g2)
    finally:
        ctx.set_transcript_device(0)


VARIANT = os.path.join(ROOT, "rust-kzg-bn254_amd", "libkzg_bn254_mi355x_boundcheck.so")
CHILD = r'''
import ctypes as C, os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import torch  # noqa: F401  (load order: tests/conftest.py)
import rust_kzg_bn254_amd  # noqa: F401
L = [m for name, m in list(sys.modules.items()) if name.endswith("_lib") and hasattr(m, "LIB_PATH")][0]
assert L.LIB_PATH == os.environ["KZG_LIB_PATH"], L.LIB_PATH
h = L.load()
n = h.kzg_bc_sites()
assert h.kzg_bc_reset_all() == 0
import pytest
rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", "-x", *%(tests)r])
counts = (C.c_ulonglong * n)()
first = (C.c_int32 * (9 * n))()
assert h.kzg_bc_read_all(counts, first) == 0
print("PYTEST_RC", int(rc))
for s in range(n):
    print("SITE", s, counts[s])
'''
WORKLOAD = ["tests/test_gpu_coset_bytes.py::test_small_case_of_every_new_kernel"]


def test_bound_checked_build_keeps_every_precondition():
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": WORKLOAD}], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "PYTEST_RC 0" in out, (out[-3000:], res.stderr[-2000:])
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert sites
    fired = {int(s[1]): int(s[2]) for s in sites if int(s[2])}
    assert not fired, fired
