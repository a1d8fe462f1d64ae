"""-m gpu: gnark-compressed G2 points decoded on the device (`kzg_g2_decompress_be_device`, `kzg_g2srs_load_compressed_be`,
`G2SRS.decompress_device`, `G2SRS.from_file`; csrc/g2_decode.h, csrc/g2decode.hip) against the host decoder `kzg_g2_decompress_be`, the
Python decoder and big-integer arithmetic on the twist.  300 points: more than one workgroup of 256, a partial last one, and no
multiple of a wave of 64.  Inputs are generated ([tau^i]_2 of a known tau, compressed by tests/g2_compress_ref.py); nothing is read
but tests/golden/g2.point.powerOf2."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import g2_compress_ref as gc
import g2_points as g2
import rust_kzg_bn254_amd as k
from pyref import P, R_
from rust_kzg_bn254_amd import _lib, helpers
from rust_kzg_bn254_amd.errors import DeserializationError, GenericError, NotOnCurveError
from rust_kzg_bn254_amd.fr import frs_from_ints

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G2_FILE = os.path.join(HERE, "golden", "g2.point.powerOf2")
TAU = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CF
N = 300
INDICES = (0, 63, 64, 255, 256, 299)
BOTH = _lib.G2_CHECK_SUBGROUP | _lib.G2_REJECT_GENERATOR


def _host(data):
    n = len(data) // 64
    out = np.zeros((max(n, 1), 16), np.uint64)
    bad = C.c_uint64(2 ** 64 - 1)
    buf = np.frombuffer(data, dtype=np.uint8)
    rc = _lib.load().kzg_g2_decompress_be(buf.ctypes.data_as(_lib.u8p), n, _lib.ptr(out), C.byref(bad))
    return rc, bad.value, out[:n]


def _device(data, flags, with_index=True):
    n = len(data) // 64
    out = np.zeros((max(n, 1), 16), np.uint64)
    bad = C.c_uint64(2 ** 64 - 1)
    buf = np.frombuffer(data, dtype=np.uint8)
    rc = _lib.load().kzg_g2_decompress_be_device(_lib.default_context().handle, buf.ctypes.data_as(_lib.u8p), n, flags, _lib.ptr(out),
                                                 C.byref(bad) if with_index else None)
    return rc, bad.value, out[:n]


def _load(data, with_index=True):
    """kzg_g2srs_load_compressed_be, then the download: (status, bad index, wire points or None)"""
    ctx = _lib.default_context()
    n = len(data) // 64
    h = C.c_void_p()
    bad = C.c_uint64(2 ** 64 - 1)
    buf = np.frombuffer(data, dtype=np.uint8)
    rc = _lib.load().kzg_g2srs_load_compressed_be(ctx.handle, buf.ctypes.data_as(_lib.u8p), n, C.byref(h), C.byref(bad) if with_index else None)
    if rc != _lib.OK:
        assert not h.value
        return rc, bad.value, None
    srs = k.G2SRS(h, n, ctx)
    try:
        return rc, bad.value, srs.g2
    finally:
        srs.close()


@pytest.fixture(scope="module")
def powers():
    """[tau^i]_2 for i <= 300 as wire points: [:300] starts with the generator, [1:] does not hold it"""
    srs = k.G2SRS.generate(TAU, N + 1)
    try:
        return srs.g2
    finally:
        srs.close()


@pytest.fixture(scope="module")
def compressed(powers):
    """the gnark bytes of those 301 points, and of their negatives"""
    return gc.compress_wire(powers), gc.compress_wire(powers, negate=True)


def _takes_swapped_branch(x):
    """the square root of x^3 + b takes the swapped branch of csrc/g2_decode.h: delta = (a0 + sqrt(norm)) / 2 is not a residue"""
    a = g2.f2add(g2.f2mul(g2.f2mul(x, x), x), g2.B)
    assert a[1] != 0
    norm = (a[0] * a[0] + a[1] * a[1]) % P
    alpha = pow(norm, (P + 1) // 4, P)
    assert alpha * alpha % P == norm
    delta = (a[0] + alpha) * pow(2, -1, P) % P
    return pow(delta, (P - 1) // 2, P) != 1


# ---- 1. the golden file -------------------------------------------------------------------------------------------------------------
def test_golden_file_equals_the_host_decoder_bit_for_bit():
    data = open(G2_FILE, "rb").read()
    rc, _, want = _host(data)
    assert rc == _lib.OK and want.shape == (28, 16)
    rc, _, got = _device(data, BOTH)
    assert rc == _lib.OK and np.array_equal(got, want)
    rc, _, got = _load(data)
    assert rc == _lib.OK and np.array_equal(got, want)
    assert np.array_equal(k.G2SRS.decompress_device(data), want)


# ---- 2. round trip ------------------------------------------------------------------------------------------------------------------
def test_round_trip_of_300_generated_points_with_both_flags(powers, compressed):
    pts = powers[:N]
    data, data_neg = compressed[0][:64 * N], compressed[1][:64 * N]
    assert np.array_equal(pts[0], helpers.g2_generator())
    swapped = sum(_takes_swapped_branch(g2.from_wire(w)[0]) for w in pts)
    assert swapped >= 64 and N - swapped >= 64, swapped
    # the loader accepts the generator at index 0
    rc, _, got = _load(data)
    assert rc == _lib.OK and np.array_equal(got, pts)
    rc, _, got = _load(data_neg)
    assert rc == _lib.OK and np.array_equal(got, gc.negate_wire(pts))
    # the decoder of untrusted points refuses it, unless told not to
    assert _device(data, BOTH)[:2] == (_lib.ERR_NOT_ON_CURVE, 0)
    rc, _, got = _device(data, _lib.G2_CHECK_SUBGROUP)
    assert rc == _lib.OK and np.array_equal(got, pts)
    rc, _, got = _device(data, 0)
    assert rc == _lib.OK and np.array_equal(got, pts)
    with pytest.raises(NotOnCurveError, match="G2 point 0 not on curve or not in the correct subgroup"):
        k.G2SRS.decompress_device(data)
    assert np.array_equal(k.G2SRS.decompress_device(data, reject_generator=False), pts)
    # without the generator: the host decoder's points
    rc, _, want = _host(compressed[0][64:])
    assert rc == _lib.OK and np.array_equal(want, powers[1:])
    rc, _, got = _device(compressed[0][64:], BOTH)
    assert rc == _lib.OK and np.array_equal(got, want)


# ---- 3. errors and the smallest index -------------------------------------------------------------------------------------------------
def _flag0(d, o, rnd): d[o] &= 0x3F                                   # noqa: E704
def _flag1(d, o, rnd): d[o] = (d[o] & 0x3F) | 0x40                    # noqa: E704
def _big_c0(d, o, rnd): d[o + 32:o + 64] = b"\xff" * 32               # noqa: E704
def _big_c1(d, o, rnd): d[o:o + 32] = bytes([d[o] | 0x3F]) + b"\xff" * 31   # noqa: E704


def _no_point(d, o, rnd):
    """an x with no point on the twist, found by stepping the last byte"""
    for t in range(1, 60):
        last = (d[o + 63] + t) % 256
        x = (int.from_bytes(bytes(d[o + 32:o + 63]) + bytes([last]), "big"), int.from_bytes(bytes([d[o] & 0x3F]) + bytes(d[o + 1:o + 32]), "big"))
        if x[0] < P and g2.f2sqrt(g2.f2add(g2.f2mul(g2.f2mul(x, x), x), g2.B)) is None:
            d[o + 63] = last
            return
    raise AssertionError("no x without a point among 59 neighbours")


def _outside(d, o, rnd):
    """a point of the twist outside the order-r subgroup"""
    pt = g2.random_twist_point(rnd)
    d[o:o + 64] = gc.compress_point(pt, negate=rnd.random() < 0.5)


KINDS = {"flag_cleared": (_flag0, _lib.ERR_DESERIALIZE), "flag_01": (_flag1, _lib.ERR_DESERIALIZE), "c0_all_ones": (_big_c0, _lib.ERR_DESERIALIZE),
         "c1_not_below_p": (_big_c1, _lib.ERR_DESERIALIZE), "no_point_of_that_x": (_no_point, _lib.ERR_NOT_ON_CURVE),
         "outside_the_subgroup": (_outside, _lib.ERR_NOT_ON_CURVE)}


def _damaged(good, i, kind, rnd):
    d = bytearray(good)
    KINDS[kind][0](d, 64 * i, rnd)
    return bytes(d)


@pytest.mark.parametrize("kind", list(KINDS))
def test_errors_equal_the_host_decoder_and_leave_the_context_usable(powers, compressed, kind):
    good, want = compressed[0][64:], powers[1:]                       # [tau^1 .. tau^300]_2: the host decoder accepts all of them
    rnd = random.Random(kind)
    for i in INDICES:
        data = _damaged(good, i, kind, rnd)
        host = _host(data)[:2]
        assert host == (KINDS[kind][1], i)
        assert _device(data, BOTH)[:2] == host, i
        assert _device(data, BOTH, with_index=False)[0] == host[0], i
        assert _load(data)[:2] == host, i
        assert _load(data, with_index=False)[0] == host[0], i
        rc, _, got = _device(good, BOTH)                                # the context still decodes the good input
        assert rc == _lib.OK and np.array_equal(got, want), i
    exc = DeserializationError if KINDS[kind][1] == _lib.ERR_DESERIALIZE else NotOnCurveError
    with pytest.raises(exc, match="G2 point 255"):
        k.G2SRS.decompress_device(_damaged(good, 255, kind, rnd))


def test_the_smallest_bad_index_is_reported_with_its_own_kind(powers, compressed):
    good = compressed[0][64:]
    rnd = random.Random(7)
    for (i, ki), (j, kj) in (((70, "no_point_of_that_x"), (290, "flag_cleared")), ((70, "flag_01"), (290, "outside_the_subgroup")),
                             ((3, "outside_the_subgroup"), (257, "c0_all_ones")), ((255, "c1_not_below_p"), (256, "no_point_of_that_x"))):
        data = _damaged(_damaged(good, i, ki, rnd), j, kj, rnd)
        host = _host(data)[:2]
        assert host == (KINDS[ki][1], i)
        assert _device(data, BOTH)[:2] == host
        assert _load(data)[:2] == host
    # with the generator in front the decoder of untrusted points names it whatever follows; the loader names the damaged point
    data = _damaged(compressed[0][:64 * N], 5, "flag_cleared", rnd)
    assert _device(data, BOTH)[:2] == _host(data)[:2] == (_lib.ERR_NOT_ON_CURVE, 0)
    assert _load(data)[:2] == (_lib.ERR_DESERIALIZE, 5)
    # without the subgroup test a point outside the subgroup decodes
    data = _damaged(good, 64, "outside_the_subgroup", rnd)
    assert _device(data, 0)[0] == _lib.OK and _device(data, _lib.G2_REJECT_GENERATOR)[0] == _lib.OK
    assert _device(data, _lib.G2_CHECK_SUBGROUP)[:2] == (_lib.ERR_NOT_ON_CURVE, 64)


# ---- 3b. more than one staged piece, more than one launch --------------------------------------------------------------------------------
# The bytes go up in pieces of 16 384 points through two pinned halves (csrc/byte_stager.h) and a kernel starts behind every 65 536.  A
# pool of 299 distinct points ([tau^1 .. tau^299]_2: one of the 300 dropped) is tiled up to the count: 299 is odd, so it divides neither a
# piece nor a launch, and a copy or launch offset that is wrong by a whole piece reads other bytes.  The yardstick is the pool's own decode
# by the same entry (compared with the host decoder above), tiled the same way.
POOL = N - 1


def _tiled(pool_bytes, item, n):
    return (pool_bytes * (n // (len(pool_bytes) // item) + 1))[:item * n]


@pytest.fixture(scope="module")
def pool(powers, compressed):
    data = compressed[0][64:64 * N]
    rc, _, out = _device(data, _lib.G2_CHECK_SUBGROUP)
    assert rc == _lib.OK and np.array_equal(out, powers[1:N])
    return data, out


@pytest.mark.parametrize("n,flags", [(32769, 0), (65538, _lib.G2_CHECK_SUBGROUP)], ids=["three_pieces_half_0_reused", "a_second_launch"])
def test_tiled_pool_across_pieces_and_launches_is_bit_equal(pool, n, flags):
    data, out = pool
    rc, _, got = _device(_tiled(data, 64, n), flags)
    assert rc == _lib.OK and np.array_equal(got, out[np.arange(n) % POOL])


def test_bad_points_in_the_second_launch_and_the_second_piece(pool):
    data, _ = pool
    rnd = random.Random(8)
    big = _tiled(data, 64, 65538)
    both = _damaged(_damaged(big, 65536, "no_point_of_that_x", rnd), 65537, "flag_cleared", rnd)
    assert _device(both, _lib.G2_CHECK_SUBGROUP)[:2] == (_lib.ERR_NOT_ON_CURVE, 65536)
    one = _damaged(big[:64 * 32769], 16384, "no_point_of_that_x", rnd)          # the first point of the second piece
    assert _device(one, 0)[:2] == (_lib.ERR_NOT_ON_CURVE, 16384)


# ---- 4. x^3 + b in Fq ----------------------------------------------------------------------------------------------------------------
def test_points_whose_y_squared_lies_in_fq():
    """x = (x0, x1) with x0^2 = (x1^3 - b1) / (3 x1) makes the u-part of x^3 + b vanish: the a1 = 0 branch of the square root, with
    y^2 a residue (y in Fq) and a non-residue (y in Fq u)."""
    residue, non_residue = [], []
    for x1 in range(1, 200):
        sq = (x1 ** 3 - g2.B[1]) * pow(3 * x1, -1, P) % P
        x0 = pow(sq, (P + 1) // 4, P)
        if x0 * x0 % P != sq:
            continue
        x = (x0, x1)
        a = g2.f2add(g2.f2mul(g2.f2mul(x, x), x), g2.B)
        assert a[1] == 0
        (residue if pow(a[0], (P - 1) // 2, P) == 1 else non_residue).append(x)
    assert len(residue) >= 8 and len(non_residue) >= 8
    xs = residue[:10] + non_residue[:10]
    data, want, pts = b"", [], []
    for i, x in enumerate(xs):
        for flag in (2, 3):
            a = g2.f2add(g2.f2mul(g2.f2mul(x, x), x), g2.B)
            y = helpers._fq2_sqrt(a[0], a[1])
            assert y is not None and (y[1] == 0) == (x in residue) and (y[0] == 0) == (x in non_residue)
            if gc.is_largest(y) != (flag == 3):
                y = (-y[0] % P, -y[1] % P)
            assert g2.on_twist((x, y))
            data += gc.compress_x(x, flag)
            want.append(g2.to_wire((x, y)))
            pts.append((x, y))
    rc, _, got = _device(data, 0)
    assert rc == _lib.OK and np.array_equal(got, np.stack(want))
    outside = [i for i, pt in enumerate(pts) if g2.mul(R_, pt) is not None]
    if outside:
        assert _device(data, _lib.G2_CHECK_SUBGROUP)[:2] == (_lib.ERR_NOT_ON_CURVE, outside[0])
    else:
        assert _device(data, _lib.G2_CHECK_SUBGROUP)[0] == _lib.OK


# ---- 5. arguments ----------------------------------------------------------------------------------------------------------------------
def test_arguments(compressed):
    lib, ctx = _lib.load(), _lib.default_context()
    good = compressed[0][64:64 * 9]
    buf = np.frombuffer(good, dtype=np.uint8)
    bp = buf.ctypes.data_as(_lib.u8p)
    out = np.zeros((8, 16), np.uint64)
    h = C.c_void_p()
    bad = C.c_uint64(0)
    assert lib.kzg_g2_decompress_be_device(ctx.handle, None, 0, BOTH, None, None) == _lib.OK
    assert lib.kzg_g2srs_load_compressed_be(ctx.handle, None, 0, C.byref(h), None) == _lib.OK and h.value
    assert lib.kzg_g2srs_len(h) == 0
    lib.kzg_g2srs_free(h)
    for args in ((None, bp, 8, BOTH, _lib.ptr(out), None), (ctx.handle, None, 8, BOTH, _lib.ptr(out), None), (ctx.handle, bp, 8, BOTH, None, None),
                 (ctx.handle, bp, 8, 4, _lib.ptr(out), None)):
        assert lib.kzg_g2_decompress_be_device(*args) == _lib.ERR_INVALID_ARG
    for args in ((None, bp, 8, C.byref(h), None), (ctx.handle, None, 8, C.byref(h), None), (ctx.handle, bp, 8, None, None)):
        assert lib.kzg_g2srs_load_compressed_be(*args) == _lib.ERR_INVALID_ARG
    # 2^28 + 1 points: refused on the host before anything of that size is allocated or read
    assert lib.kzg_g2_decompress_be_device(ctx.handle, bp, (1 << 28) + 1, BOTH, _lib.ptr(out), C.byref(bad)) == _lib.ERR_TOO_LARGE
    h = C.c_void_p(1)
    assert lib.kzg_g2srs_load_compressed_be(ctx.handle, bp, (1 << 28) + 1, C.byref(h), C.byref(bad)) == _lib.ERR_TOO_LARGE and not h.value
    # a _begin on slot 0 in flight
    srs = k.SRS.generate(TAU, 64)
    try:
        sc = np.ascontiguousarray(frs_from_ints(list(range(1, 65))))
        xy = np.zeros(8, np.uint64)
        inf = C.c_uint8(0)
        assert lib.kzg_msm_g1_srs_begin(ctx.handle, srs.handle, 0, _lib.ptr(sc), 64, 0) == _lib.OK
        try:
            assert lib.kzg_g2_decompress_be_device(ctx.handle, bp, 8, BOTH, _lib.ptr(out), None) == _lib.ERR_INVALID_ARG
            h = C.c_void_p(1)
            assert lib.kzg_g2srs_load_compressed_be(ctx.handle, bp, 8, C.byref(h), None) == _lib.ERR_INVALID_ARG and not h.value
        finally:
            assert lib.kzg_msm_g1_srs_end(ctx.handle, 0, _lib.ptr(xy), C.byref(inf), None) == _lib.OK
        assert lib.kzg_g2_decompress_be_device(ctx.handle, bp, 8, BOTH, _lib.ptr(out), None) == _lib.OK
        assert np.array_equal(out, _host(good)[2])
    finally:
        srs.close()
    with pytest.raises(DeserializationError):
        k.G2SRS.decompress_device(b"")
    with pytest.raises(DeserializationError):
        k.G2SRS.decompress_device(good[:-1])


# ---- 6. G2SRS.from_file -----------------------------------------------------------------------------------------------------------------
def test_from_file_with_an_offset(powers, compressed, tmp_path):
    path = str(tmp_path / "g2.powers")
    with open(path, "wb") as f:
        f.write(compressed[0][:64 * N])
    whole = k.G2SRS.from_file(path, N)
    window = k.G2SRS.from_file(path, 100, first_power=137, offset_points=137)
    generated = k.G2SRS.generate(TAU, N)
    try:
        assert len(whole) == N and np.array_equal(whole.g2, powers[:N])
        assert len(window) == 100 and window.first_power == 137 and np.array_equal(window.g2, powers[137:237])
        with pytest.raises(GenericError, match="Expected 100 points, only read 99"):
            k.G2SRS.from_file(path, 100, offset_points=201)
        with pytest.raises(GenericError, match="Expected 301 points, only read 300"):
            k.G2SRS.from_file(path, N + 1)
        rnd = random.Random(6)
        poly = k.PolynomialCoeffForm(frs_from_ints([rnd.randrange(R_) for _ in range(64)]))
        kzg = k.KZG.new()
        assert np.array_equal(kzg.commit_g2_coeff_form(poly, whole), kzg.commit_g2_coeff_form(poly, generated))
    finally:
        whole.close(); window.close(); generated.close()
    bad = bytearray(compressed[0][:64 * N])
    bad[64 * 200] &= 0x3F
    with open(path, "wb") as f:
        f.write(bytes(bad))
    with pytest.raises(DeserializationError, match="G2 point 200: not a compressed finite point below the modulus"):
        k.G2SRS.from_file(path, N)
    with pytest.raises(DeserializationError, match="G2 point 63:"):
        k.G2SRS.from_file(path, 100, offset_points=137)
    again = k.G2SRS.from_file(path, 200)                                # the points in front of the damaged one load
    try:
        assert np.array_equal(again.g2, powers[:200])
    finally:
        again.close()
