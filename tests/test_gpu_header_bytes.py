"""-m gpu: blob headers verified and located from their serialized bytes (`kzg_verify_length_proof_batch_bytes`,
`kzg_verify_length_proof_batch_locate_bytes`, `kzg_header_items_decode_be`).

The pool is that of tests/test_gpu_header_batch.py: headers from a known tau over a setup of order N = 2^10, C = [f]_1, C2 = [f]_2,
pi2 = [tau^(N-d) f]_2.  Their bytes are made in Python (tests/g2_compress_ref.py for G2, the same sign rule on pyref's integers for G1), not
by the library's encoder.  The reference of every verdict, weight and good / bad map is the decoded entry on the wire points the bytes
were made from."""
import ctypes as C
import random

import numpy as np
import pytest

import g2_compress_ref as ref
import g2_points as g2
import pyref
from pyref import P, R_

pytestmark = pytest.mark.gpu

N = 1024
LENS = (1, 4, 1024)
POOL = 260
HALF = (P - 1) // 2
ID32, ID64 = b"\x40" + bytes(31), b"\x40" + bytes(63)


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    return k


def g1_mul(s):
    return pyref.point_to_wire(pyref.ec_mul(s % R_, (1, 2)) if s % R_ else None)


def g2_mul(k, s):
    return k.helpers.g2_mul_generator(pyref.fr_to_mont(s % R_))


def compress_g1(wire) -> bytes:
    pt = pyref.point_from_wire(wire)
    if pt is None:
        return ID32
    b = bytearray(pt[0].to_bytes(32, "big"))
    b[0] |= 0xC0 if pt[1] > HALF else 0x80
    return bytes(b)


def compress_g2(wire) -> bytes:
    return ref.compress_wire(wire) if np.asarray(wire).any() else ID64


class Env:
    pass


@pytest.fixture(scope="module")
def env(k):
    """the pool by its scalars, as wire points and as bytes: header i of length d is (c[i], c2[i], pi2[d][i])"""
    e = Env()
    rnd = random.Random(2024)
    e.tau = rnd.randrange(2, R_)
    e.shift_scalar = {d: pow(e.tau, N - d, R_) for d in LENS}
    e.shifts = {d: g1_mul(s) for d, s in e.shift_scalar.items()}
    e.f = [rnd.randrange(1, R_) for _ in range(POOL)]
    e.c = np.stack([g1_mul(f) for f in e.f])
    e.c2 = np.stack([g2_mul(k, f) for f in e.f])
    e.pi2 = {d: np.stack([g2_mul(k, e.shift_scalar[d] * f) for f in e.f]) for d in LENS}
    e.c_be = [compress_g1(w) for w in e.c]
    e.c2_be = [compress_g2(w) for w in e.c2]
    e.pi2_be = {d: [compress_g2(w) for w in e.pi2[d]] for d in LENS}
    assert {b[0] >> 6 for b in e.c2_be} == {2, 3} and {b[0] >> 6 for b in e.c_be} == {2, 3}
    e.ctx = k._lib.Context(0)
    rng = random.Random(77)
    e.outside = g2.random_twist_point(rng)                          # on the twist, outside the subgroup
    assert g2.on_twist(e.outside) and g2.mul(R_, e.outside) is not None
    x = 5
    while g2.f2sqrt(g2.f2add(g2.f2mul(g2.f2mul((x, 1), (x, 1)), (x, 1)), g2.B)) is not None:
        x += 1
    e.x2_no_point = (x, 1)
    x = 1
    while pow((x * x * x + 3) % P, (P - 1) // 2, P) == 1:
        x += 1
    e.x1_no_point = x
    return e


class Hdr:
    """`count` pool headers with these lengths: wire points and byte lists side by side, edited together or apart"""

    def __init__(self, env, lens):
        n = len(lens)
        self.lens = list(lens)
        self.c, self.c2 = env.c[:n].copy(), env.c2[:n].copy()
        self.pi2 = np.stack([env.pi2[d][i] for i, d in enumerate(lens)]) if n else np.zeros((0, 16), np.uint64)
        self.c_be, self.c2_be = list(env.c_be[:n]), list(env.c2_be[:n])
        self.pi2_be = [env.pi2_be[d][i] for i, d in enumerate(lens)]

    def set(self, i, c=None, c2=None, pi2=None):
        """replace elements of header i by other wire points, in both forms"""
        if c is not None:
            self.c[i] = c; self.c_be[i] = compress_g1(c)
        if c2 is not None:
            self.c2[i] = c2; self.c2_be[i] = compress_g2(c2)
        if pi2 is not None:
            self.pi2[i] = pi2; self.pi2_be[i] = compress_g2(pi2)

    def bytes(self):
        return b"".join(self.c_be), b"".join(self.c2_be), b"".join(self.pi2_be)

    def wire(self):
        return self.c, self.c2, self.pi2


def three_groups(count):
    lens = [1 if i % 2 else 4 for i in range(count)]
    lens[count // 2] = 1024
    return lens


def fused(k, env, h, weights=None, return_weights=False):
    return k.verifier.verify_length_proof_batch_bytes(*h.bytes(), h.lens, env.shifts, weights=weights, ctx=env.ctx, return_weights=return_weights)


def decoded(k, env, h, weights=None):
    return k.verifier.verify_length_proof_batch(*h.wire(), h.lens, env.shifts, weights=weights, ctx=env.ctx)


def raw(k, env, h, entry="verify", nulls=(), count=None, gi=None, n_groups=None):
    """the C-ABI call itself: (status, out_ok or bad groups, bad_index, bad_array)"""
    L = k._lib
    bufs = [np.frombuffer(b, np.uint8) for b in h.bytes()]
    lens = np.ascontiguousarray(h.lens, np.uint64)
    sl = np.ascontiguousarray(list(env.shifts), np.uint64)
    sp = np.ascontiguousarray(np.stack(list(env.shifts.values())), np.uint64)
    u8 = lambda a: a.ctypes.data_as(L.u8p)                                      # noqa: E731
    a = {"c": u8(bufs[0]), "c2": u8(bufs[1]), "pi2": u8(bufs[2]), "lens": L.ptr(lens), "sl": L.ptr(sl), "sp": L.ptr(sp)}
    ok, bad, arr = L.i32(-5), C.c_uint64(2 ** 64 - 1), L.i32(-5)
    a["out"] = C.byref(ok)
    n = len(h.lens) if count is None else count
    if entry == "verify":
        for name in nulls:
            a[name] = None
        rc = L.load().kzg_verify_length_proof_batch_bytes(env.ctx.handle, a["c"], a["c2"], a["pi2"], a["lens"], n, a["sl"], a["sp"], len(sl), None, a["out"], None,
                                                          C.byref(bad), C.byref(arr))
        return rc, ok.value, bad.value, arr.value
    gi = np.arange(len(h.lens), dtype=np.uint64) if gi is None else np.ascontiguousarray(gi, np.uint64)
    n_groups = len(h.lens) if n_groups is None else n_groups
    good = np.full(max(n_groups, 1), 9, np.uint8)
    n_bad, checks = L.sz(99), L.sz(99)
    a["gi"], a["good"], a["out"] = L.ptr(gi), u8(good), C.byref(n_bad)
    for name in nulls:
        a[name] = None
    rc = L.load().kzg_verify_length_proof_batch_locate_bytes(env.ctx.handle, a["c"], a["c2"], a["pi2"], a["lens"], n, a["sl"], a["sp"], len(sl), None, a["gi"], n_groups,
                                                             a["good"], a["out"], C.byref(checks), C.byref(bad), C.byref(arr))
    return rc, n_bad.value, bad.value, arr.value


# ---- the decode entry -----------------------------------------------------------------------------------------------------------------
def test_decode_is_bit_equal_to_the_points_and_encode_inverts_it(k, env):
    h = Hdr(env, three_groups(POOL))
    h.set(3, c=np.zeros(8, np.uint64), c2=np.zeros(16, np.uint64), pi2=np.zeros(16, np.uint64))
    h.set(70, pi2=np.zeros(16, np.uint64))
    h.set(71, c2=g2_mul(k, 1))                                      # the generator is an element like any other
    c, c2, pi2 = k.verifier.decode_header_items(*h.bytes(), ctx=env.ctx)
    assert np.array_equal(c, h.c) and np.array_equal(c2, h.c2) and np.array_equal(pi2, h.pi2)
    assert k.verifier.encode_header_items(c, c2, pi2) == h.bytes()


# ---- accepts --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouping", ["one", "three"])
@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 257])          # the wave (64) and workgroup (256) edges
def test_honest_batches_with_the_weights_of_the_decoded_entry(k, env, count, grouping):
    h = Hdr(env, [4] * count if grouping == "one" else three_groups(count))
    ok, w = fused(k, env, h, return_weights=True)
    want = k.verifier.compute_header_batch_weights(*h.wire(), h.lens, env.shifts)
    assert ok is True and np.array_equal(w, want)                    # bit for bit
    assert decoded(k, env, h) is True
    own = pyref.frs_to_mont([random.Random(count).randrange(1, 2 ** 128) for _ in range(count + 1)])
    ok, w = fused(k, env, h, weights=own, return_weights=True)
    assert ok is True and np.array_equal(w, own)


def test_identity_headers(k, env):
    h = Hdr(env, three_groups(9))
    z8, z16 = np.zeros(8, np.uint64), np.zeros(16, np.uint64)
    h.set(4, c=z8, c2=z16, pi2=z16)                                 # the zero polynomial among honest headers
    assert h.c2_be[4] == ID64 and h.c_be[4] == ID32
    ok, w = fused(k, env, h, return_weights=True)
    assert ok is True and decoded(k, env, h) is True
    assert np.array_equal(w, k.verifier.compute_header_batch_weights(*h.wire(), h.lens, env.shifts))
    h.set(4, pi2=env.pi2[4][4])                                     # C2 the identity and pi2 not
    assert decoded(k, env, h) is False and fused(k, env, h) is False
    z = Hdr(env, [1, 4, 1024])
    for i in range(3):
        z.set(i, c=z8, c2=z16, pi2=z16)
    assert fused(k, env, z) is True                                 # nothing but identities


# ---- equation rejects -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [0, 63, 64, 129])                   # 129 = count - 1
def test_another_subgroup_point_as_the_proof_is_rejected_as_by_the_decoded_entry(k, env, pos):
    h = Hdr(env, [4] * 130)
    h.set(pos, pi2=env.pi2[4][200])
    got, w = fused(k, env, h, return_weights=True)
    assert got is False and decoded(k, env, h) is False
    assert np.array_equal(w, k.verifier.compute_header_batch_weights(*h.wire(), h.lens, env.shifts))
    assert fused(k, env, Hdr(env, [4] * 130)) is True


# ---- decode errors --------------------------------------------------------------------------------------------------------------------
def bad_element(env, array, kind):
    """bytes of one element that fails with `kind`, and the status it fails with"""
    L_DES, L_OFF = -15, -16
    if array == "c":
        x = {"flag00": 5, "stray": 0, "x>=p": P, "no point": env.x1_no_point}[kind]
        b = bytearray(x.to_bytes(32, "big"))
        if kind == "stray":
            b[31] = 1
        b[0] |= {"flag00": 0x00, "stray": 0x40}.get(kind, 0x80)
        return bytes(b), L_DES if kind != "no point" else L_OFF
    good = g2.from_wire(env.c2[7])
    if kind == "flag00":
        return ref.compress_x(good[0], 0), L_DES
    if kind == "stray":
        return b"\x40" + bytes(40) + b"\x01" + bytes(22), L_DES     # 0b01 with a bit set in X.A0
    if kind == "x>=p":
        return ref.compress_x((P, 1), 2), L_DES                     # X.A0 = p, X.A1 below it
    if kind == "x1>=p":
        return ref.compress_x((1, P), 3), L_DES
    if kind == "no point":
        return ref.compress_x(env.x2_no_point, 2), L_OFF
    assert kind == "outside"
    return ref.compress_point(env.outside), L_OFF


CASES = [("c", kd) for kd in ("flag00", "stray", "x>=p", "no point")] + \
        [(a, kd) for a in ("c2", "pi2") for kd in ("flag00", "stray", "x>=p", "x1>=p", "no point", "outside")]


@pytest.mark.parametrize("array,kind", CASES, ids=["%s-%s" % c for c in CASES])
def test_each_kind_of_bad_element_in_each_array(k, env, array, kind):
    L = k._lib
    assert (L.ERR_DESERIALIZE, L.ERR_NOT_ON_CURVE) == (-15, -16)
    b, status = bad_element(env, array, kind)
    for pos in (0, 64, 65):                                         # first, the first lane of the second wave's headers, last
        h = Hdr(env, three_groups(66))
        getattr(h, array + "_be")[pos] = b
        for entry in ("verify", "locate"):
            assert raw(k, env, h, entry) == (status, -5 if entry == "verify" else 99, pos, ("c", "c2", "pi2").index(array)), (pos, entry)
    assert raw(k, env, Hdr(env, three_groups(66))) == (L.OK, 1, 2 ** 64 - 1, -5)          # the context is usable after the errors
    with pytest.raises(k.errors.DeserializationError if status == -15 else k.errors.NotOnCurveError,
                       match="%s 65" % {"c": "commitment", "c2": "length commitment", "pi2": "length proof"}[array]):
        fused(k, env, h)
    with pytest.raises(k.errors.KzgError, match=" 65"):
        k.verifier.decode_header_items(*h.bytes(), ctx=env.ctx)


def test_which_bad_element_is_reported(k, env):
    des, off = bad_element(env, "c2", "flag00")[0], bad_element(env, "c2", "outside")[0]
    # a bad commitment beats a bad G2 element of an earlier header
    h = Hdr(env, [4] * 70)
    h.c2_be[2] = des
    h.c_be[66] = bad_element(env, "c", "no point")[0]
    assert raw(k, env, h) == (-16, -5, 66, 0)
    # pi2 of header 3 beats C2 of header 5, with its own kind
    h = Hdr(env, [4] * 70)
    h.pi2_be[3] = off
    h.c2_be[5] = des
    assert raw(k, env, h) == (-16, -5, 3, 2)
    # of two bad elements of one array the smaller index wins, across waves and with its own kind
    h = Hdr(env, [4] * 70)
    h.c2_be[69] = off
    h.c2_be[64] = des
    assert raw(k, env, h) == (-15, -5, 64, 1)
    # C2 beats pi2 within one header
    h = Hdr(env, [4] * 70)
    h.pi2_be[33] = des
    h.c2_be[33] = off
    assert raw(k, env, h) == (-16, -5, 33, 1)
    # a shift off the curve beats them all: the host tests it before any launch
    shifts = dict(env.shifts)
    bad_shift = shifts[4].copy()
    bad_shift[4] ^= 1
    shifts[4] = bad_shift
    with pytest.raises(k.errors.NotOnCurveError, match="shift 1"):
        k.verifier.verify_length_proof_batch_bytes(*h.bytes(), h.lens, shifts, ctx=env.ctx)
    assert fused(k, env, Hdr(env, [4] * 70)) is True


# ---- locate ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bad", [1, 3])
@pytest.mark.parametrize("count", [65, 257])
def test_locate_gives_the_map_and_the_checks_of_the_decoded_entry(k, env, count, n_bad):
    h = Hdr(env, three_groups(count))
    bad = [count - 1] if n_bad == 1 else [0, 63, count - 1]
    h.set(count - 1, pi2=env.pi2[h.lens[count - 1]][200])
    if n_bad == 3:
        h.set(63, c2=env.c2[201])
        h.set(0, c=env.c[202])
    V = k.verifier
    good, checks = V.locate_bad_headers_bytes(*h.bytes(), h.lens, env.shifts, ctx=env.ctx, groups="item")
    want, want_checks = V.locate_bad_headers(*h.wire(), h.lens, env.shifts, ctx=env.ctx, groups="item")
    assert np.array_equal(good, want) and checks == want_checks
    assert sorted(np.flatnonzero(~good)) == sorted(bad)
    coarse = [i // 8 for i in range(count)]
    n_groups = coarse[-1] + 2                                       # the last group is empty
    good, checks = V.locate_bad_headers_bytes(*h.bytes(), h.lens, env.shifts, ctx=env.ctx, groups=coarse, n_groups=n_groups)
    want, want_checks = V.locate_bad_headers(*h.wire(), h.lens, env.shifts, ctx=env.ctx, groups=coarse, n_groups=n_groups)
    assert np.array_equal(good, want) and checks == want_checks
    assert sorted(np.flatnonzero(~good)) == sorted({i // 8 for i in bad})
    own = pyref.frs_to_mont([random.Random(count + n_bad).randrange(1, 2 ** 128) for _ in range(count + 1)])
    assert np.array_equal(V.locate_bad_headers_bytes(*h.bytes(), h.lens, env.shifts, weights=own, ctx=env.ctx)[0],
                          V.locate_bad_headers(*h.wire(), h.lens, env.shifts, weights=own, ctx=env.ctx)[0])
    honest = Hdr(env, three_groups(count))
    good, checks = V.locate_bad_headers_bytes(*honest.bytes(), honest.lens, env.shifts, ctx=env.ctx)
    assert good.all() and checks == 1


# ---- more headers than one decode launch takes ----------------------------------------------------------------------------------------
def test_a_batch_one_header_above_a_decode_launch(k, env):
    """32 768 headers are 65 536 G2 elements, one launch of the decode kernel; header 32 768 is the first of the second launch and, for the
    stager, the first header of the third pair of staged pieces"""
    count = 32769
    idx = np.arange(count) % POOL
    c_be = np.frombuffer(b"".join(env.c_be), np.uint8).reshape(POOL, 32)[idx]
    c2_be = np.frombuffer(b"".join(env.c2_be), np.uint8).reshape(POOL, 64)[idx]
    pi2_be = np.frombuffer(b"".join(env.pi2_be[4]), np.uint8).reshape(POOL, 64)[idx]
    lens = [4] * count
    V = k.verifier
    assert V.verify_length_proof_batch_bytes(c_be, c2_be, pi2_be, lens, env.shifts, ctx=env.ctx) is True
    bad = c2_be.copy()
    bad[count - 1] = np.frombuffer(bad_element(env, "c2", "outside")[0], np.uint8)
    with pytest.raises(k.errors.NotOnCurveError, match="length commitment 32768"):
        V.verify_length_proof_batch_bytes(c_be, bad, pi2_be, lens, env.shifts, ctx=env.ctx)
    wrong = pi2_be.copy()
    wrong[count - 1] = pi2_be[5]                                    # a subgroup point, the wrong one: the equation fails
    assert V.verify_length_proof_batch_bytes(c_be, c2_be, wrong, lens, env.shifts, ctx=env.ctx) is False


def test_a_batch_above_a_decode_launch_tiled_with_an_odd_period(k, env):
    """The same count with the headers in a sequence of period 1 021 over the pool (header i is pool header (i mod 1 021) mod 260): 1 021
    is odd, so it divides neither a staged piece (16 384 headers) nor a launch, and a copy or launch offset that is wrong by a whole piece
    reads other bytes (16 384 = 48 mod 1 021, and neither 48 nor 48 - 1 021 is a multiple of 260).  One stager (csrc/byte_stager.h) takes
    2 x 3 G2 pieces and then the 2 pieces of the commitments, the first of them in a half that a G2 piece used last."""
    count = 32769
    idx = (np.arange(count) % 1021) % POOL
    c_be = np.frombuffer(b"".join(env.c_be), np.uint8).reshape(POOL, 32)[idx]
    c2_be = np.frombuffer(b"".join(env.c2_be), np.uint8).reshape(POOL, 64)[idx]
    pi2_be = np.frombuffer(b"".join(env.pi2_be[4]), np.uint8).reshape(POOL, 64)[idx]
    lens = [4] * count
    V = k.verifier
    assert V.verify_length_proof_batch_bytes(c_be, c2_be, pi2_be, lens, env.shifts, ctx=env.ctx) is True
    bad = c2_be.copy()
    bad[16384] = np.frombuffer(bad_element(env, "c2", "no point")[0], np.uint8)       # the first header of the second pair of pieces
    with pytest.raises(k.errors.NotOnCurveError, match="length commitment 16384"):
        V.verify_length_proof_batch_bytes(c_be, bad, pi2_be, lens, env.shifts, ctx=env.ctx)
    wrong = pi2_be.copy()
    wrong[32768] = pi2_be[5]                                        # a subgroup point, the wrong one: the equation fails
    assert not np.array_equal(wrong[32768], pi2_be[32768])
    assert V.verify_length_proof_batch_bytes(c_be, c2_be, wrong, lens, env.shifts, ctx=env.ctx) is False


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_in_their_order(k, env):
    L = k._lib
    lib = k.load()
    h = Hdr(env, three_groups(5))
    for entry in ("verify", "locate"):
        for name in ("c", "c2", "pi2", "lens", "sl", "sp", "out") + (("gi", "good") if entry == "locate" else ()):
            assert raw(k, env, h, entry, nulls=(name,))[0] == L.ERR_INVALID_ARG, (entry, name)
        # count > 2^20: refused on the host, nothing of that size is read (the length check of row 2 runs first, so the lengths are real)
        big = Hdr(env, [4] * 4)
        big.lens = [4] * (2 ** 20 + 1)
        assert raw(k, env, big, entry, gi=np.zeros(2 ** 20 + 1, np.uint64), n_groups=1)[0] == L.ERR_TOO_LARGE
        # count = 0: accepted, no device work
        empty = Hdr(env, [])
        rc, out, bad, arr = raw(k, env, empty, entry, n_groups=0)
        assert (rc, out, bad, arr) == (L.OK, 1 if entry == "verify" else 0, 2 ** 64 - 1, -5)
        assert raw(k, env, h, entry)[0] == L.OK
    assert k.verifier.verify_length_proof_batch_bytes(b"", b"", b"", [], env.shifts, ctx=env.ctx) is True
    bufs = [np.frombuffer(b, np.uint8) for b in h.bytes()]
    u8 = lambda a: a.ctypes.data_as(L.u8p)                                      # noqa: E731
    o8, o16a, o16b = np.zeros((5, 8), np.uint64), np.zeros((5, 16), np.uint64), np.zeros((5, 16), np.uint64)
    # 2^20 + 1 headers: refused on the host before anything of that size is allocated or read
    assert lib.kzg_header_items_decode_be(env.ctx.handle, u8(bufs[0]), u8(bufs[1]), u8(bufs[2]), 2 ** 20 + 1, L.ptr(o8), L.ptr(o16a), L.ptr(o16b), None,
                                          None) == L.ERR_TOO_LARGE
    for null in range(6):
        args = [u8(bufs[0]), u8(bufs[1]), u8(bufs[2]), 5, L.ptr(o8), L.ptr(o16a), L.ptr(o16b)]
        args[null if null < 3 else null + 1] = None
        assert lib.kzg_header_items_decode_be(env.ctx.handle, *args, None, None) == L.ERR_INVALID_ARG
    # a bad element with both out-pointers null
    hb = Hdr(env, three_groups(5))
    hb.c2_be[2] = bad_element(env, "c2", "outside")[0]
    bb = [np.frombuffer(b, np.uint8) for b in hb.bytes()]
    lens, sl = np.ascontiguousarray(hb.lens, np.uint64), np.ascontiguousarray(list(env.shifts), np.uint64)
    sp = np.ascontiguousarray(np.stack(list(env.shifts.values())), np.uint64)
    ok = L.i32(-5)
    assert lib.kzg_verify_length_proof_batch_bytes(env.ctx.handle, u8(bb[0]), u8(bb[1]), u8(bb[2]), L.ptr(lens), 5, L.ptr(sl), L.ptr(sp), 3, None, C.byref(ok), None,
                                                   None, None) == L.ERR_NOT_ON_CURVE and ok.value == -5
    # a _begin on slot 0 in flight
    srs = k.SRS.generate(env.tau, 64, ctx=env.ctx)
    sc = np.ascontiguousarray(pyref.frs_to_mont(list(range(1, 65))))
    xy, inf = np.zeros(8, np.uint64), C.c_uint8(0)
    assert lib.kzg_msm_g1_srs_begin(env.ctx.handle, srs.handle, 0, L.ptr(sc), 64, 0) == L.OK
    try:
        assert raw(k, env, h, "verify") == (L.ERR_INVALID_ARG, -5, 2 ** 64 - 1, -5)
        assert raw(k, env, h, "locate") == (L.ERR_INVALID_ARG, 99, 2 ** 64 - 1, -5)
        assert lib.kzg_header_items_decode_be(env.ctx.handle, u8(bufs[0]), u8(bufs[1]), u8(bufs[2]), 5, L.ptr(o8), L.ptr(o16a), L.ptr(o16b), None, None) == L.ERR_INVALID_ARG
    finally:
        assert lib.kzg_msm_g1_srs_end(env.ctx.handle, 0, L.ptr(xy), C.byref(inf), None) == L.OK
    assert raw(k, env, h, "verify") == (L.OK, 1, 2 ** 64 - 1, -5)


def test_the_trace_names_decode_and_digests():
    """KZG_VB_TRACE is read when the library loads: a child process"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    body = r'''
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import torch  # noqa: F401  (load order: tests/conftest.py)
import numpy as np
import rust_kzg_bn254_amd as k
import pyref
V = k.verifier
g1 = pyref.point_to_wire((1, 2))
gen = k.helpers.g2_mul_generator(pyref.fr_to_mont(1))
c, c2, p2 = V.encode_header_items(np.stack([g1] * 3), np.stack([gen] * 3), np.stack([gen] * 3))
print("RESULT", V.verify_length_proof_batch_bytes(c, c2, p2, [1024] * 3, {1024: g1}), bool(V.locate_bad_headers_bytes(c, c2, p2, [1024] * 3, {1024: g1})[0].all()))
''' % {"root": root}
    res = subprocess.run([sys.executable, "-c", body], capture_output=True, text=True, timeout=300, env=dict(os.environ, KZG_VB_TRACE="1"), cwd=root)
    assert res.returncode == 0 and "RESULT True True" in res.stdout, (res.stdout[-2000:], res.stderr[-2000:])
    lines = [ln for ln in res.stderr.splitlines() if "verify_length_proof_batch" in ln]
    assert len(lines) == 2 and all("decode" in ln and "digests" in ln for ln in lines), res.stderr[-2000:]
    assert "verify_length_proof_batch_bytes" in lines[0] and "verify_length_proof_batch_locate_bytes" in lines[1]
