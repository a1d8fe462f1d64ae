"""-m gpu: batched verification of blob headers (`kzg_verify_length_proof_batch`) and the device subgroup test (`kzg_g2_check_subgroup`).

Headers come from a known tau over a setup of order N = 2^10: C = [f]_1, C2 = [f]_2, pi2 = [tau^(N-d) f]_2 for a random scalar f, made
by the host's fixed-base multiplication (no MSM).  The reference of every accept / reject decision is the single-call
`kzg_verify_length_proof` on the same items."""
import ctypes as C
import random

import numpy as np
import pytest

import g2_points as g2
import pyref
from pyref import R_

pytestmark = pytest.mark.gpu

N = 1024
LENS = (1, 4, 1024)
POOL = 260
OK, INVALID, NOT_POW2, TOO_LARGE, NOT_ON_CURVE, G1_OFF, G2_OFF = 0, -1, -7, -11, -16, -17, -18


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    return k


def g1_mul(s):
    return pyref.point_to_wire(pyref.ec_mul(s % R_, (1, 2)) if s % R_ else None)


def g2_mul(k, s):
    return k.helpers.g2_mul_generator(pyref.fr_to_mont(s % R_))


class Env:
    pass


@pytest.fixture(scope="module")
def env(k):
    """a pool of honest headers by their scalars: header i of length d is (c[i], c2[i], pi2[d][i])"""
    e = Env()
    rnd = random.Random(2024)
    e.tau = rnd.randrange(2, R_)
    e.shift_scalar = {d: pow(e.tau, N - d, R_) for d in LENS}
    e.shifts = {d: g1_mul(s) for d, s in e.shift_scalar.items()}
    assert pyref.point_from_wire(e.shifts[N]) == (1, 2)             # d = N: the shift is the generator
    e.f = [rnd.randrange(1, R_) for _ in range(POOL)]
    e.c = np.stack([g1_mul(f) for f in e.f])
    e.c2 = np.stack([g2_mul(k, f) for f in e.f])
    e.pi2 = {d: np.stack([g2_mul(k, e.shift_scalar[d] * f) for f in e.f]) for d in LENS}
    e.ctx = k._lib.Context(0)
    return e


def honest(env, lens):
    """(commitments, length commitments, length proofs, lens) of the first len(lens) pool headers with these lengths"""
    n = len(lens)
    return env.c[:n].copy(), env.c2[:n].copy(), np.stack([env.pi2[d][i] for i, d in enumerate(lens)]) if n else np.zeros((0, 16), np.uint64), list(lens)


def three_groups(count):
    """lengths 1 and 4 alternating, and ONE header of length 1024"""
    lens = [1 if i % 2 else 4 for i in range(count)]
    lens[count // 2] = 1024
    return lens


def batch(k, env, hdr, weights=None, ctx=None, shifts=None):
    c, c2, pi2, lens = hdr
    return k.verifier.verify_length_proof_batch(c, c2, pi2, lens, shifts or env.shifts, weights=weights, ctx=ctx or env.ctx)


def reference(k, env, hdr, only=None):
    """all(kzg_verify_length_proof(header_i)); `only`: the headers that differ from the pool's honest ones (the others are known)"""
    c, c2, pi2, lens = hdr
    idx = range(len(lens)) if only is None else only
    return all(k.verifier.verify_length_proof(c[i], c2[i], pi2[i], env.shifts[lens[i]]) for i in idx)


def raw(k, env, hdr, shift_lens=None, shift_pts=None, weights=None, ctx=None, count=None, nulls=()):
    """the C-ABI call itself: (status, out_ok, bad_index)"""
    L = k._lib
    c, c2, pi2, lens = hdr
    c = np.ascontiguousarray(c, np.uint64); c2 = np.ascontiguousarray(c2, np.uint64); pi2 = np.ascontiguousarray(pi2, np.uint64)
    lens = np.ascontiguousarray(lens, np.uint64)
    sl = np.ascontiguousarray(list(env.shifts) if shift_lens is None else shift_lens, np.uint64)
    sp = np.ascontiguousarray(np.stack(list(env.shifts.values())) if shift_pts is None else shift_pts, np.uint64)
    ok, bad = L.i32(-5), C.c_uint64(2 ** 64 - 1)
    args = {"c": L.ptr(c), "c2": L.ptr(c2), "pi2": L.ptr(pi2), "lens": L.ptr(lens), "sl": L.ptr(sl) if sl.size else None, "sp": L.ptr(sp) if sp.size else None}
    for name in nulls:
        args[name] = None
    w = None if weights is None else np.ascontiguousarray(weights, np.uint64)
    rc = L.load().kzg_verify_length_proof_batch((ctx or env.ctx).handle, args["c"], args["c2"], args["pi2"], args["lens"], len(lens) if count is None else count,
                                                args["sl"], args["sp"], len(sl), None if w is None else L.ptr(w), C.byref(ok), C.byref(bad))
    return rc, ok.value, bad.value


# ---- accepts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouping", ["one", "three"])
@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 257])          # the wave (64) and workgroup (256) tile edges
def test_accepts_honest_batches(k, env, count, grouping):
    lens = [4] * count if grouping == "one" else three_groups(count)
    hdr = honest(env, lens)
    assert reference(k, env, hdr) is True
    assert batch(k, env, hdr) is True


def test_accepts_identities_and_duplicates(k, env):
    c, c2, pi2, lens = honest(env, three_groups(9))
    c[4] = 0; c2[4] = 0; pi2[4] = 0                                 # the zero polynomial
    hdr = (c, c2, pi2, lens)
    assert reference(k, env, hdr, only=[4]) is True
    assert batch(k, env, hdr) is True
    c, c2, pi2, lens = honest(env, [4] * 6)
    c[5], c2[5], pi2[5] = c[1], c2[1], pi2[1]                       # the same header twice
    assert batch(k, env, (c, c2, pi2, lens)) is True
    z = (np.zeros((3, 8), np.uint64), np.zeros((3, 16), np.uint64), np.zeros((3, 16), np.uint64), [1, 4, 1024])
    assert batch(k, env, z) is True                                 # nothing but identities: every sum is the identity
    assert batch(k, env, honest(env, [])) is True                   # count = 0


# ---- rejects ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [0, 63, 64])                        # 64 is the last of 65: the first lane of the second tile
@pytest.mark.parametrize("what", ["C", "C2", "pi2", "d"])
def test_rejects_one_bad_header(k, env, pos, what):
    c, c2, pi2, lens = honest(env, [4] * 65)
    if what == "C":
        c[pos] = env.c[200]
    elif what == "C2":
        c2[pos] = env.c2[200]
    elif what == "pi2":
        pi2[pos] = env.pi2[4][200]
    else:
        lens[pos] = 1                                               # another listed length: the proof is for d = 4
    hdr = (c, c2, pi2, lens)
    want = reference(k, env, hdr, only=[pos])
    assert want is False
    assert batch(k, env, hdr) is want


def _ones(count):
    return pyref.frs_to_mont([1] * (count + 1))


def test_the_weights_are_per_item(k, env):
    q = 0xABCDEF0123456789
    s = env.shift_scalar[4]
    # pi2_A + Q, pi2_B - Q: the errors cancel in an unweighted sum
    c, c2, pi2, lens = honest(env, [4] * 5)
    pi2[1] = g2_mul(k, s * env.f[1] + q)
    pi2[3] = g2_mul(k, s * env.f[3] - q)
    hdr = (c, c2, pi2, lens)
    assert reference(k, env, hdr, only=[1, 3]) is False
    assert batch(k, env, hdr, weights=_ones(5)) is True
    assert batch(k, env, hdr) is False
    # the same pair on C2 covers the first equation (and, through e(T, C2), the second)
    c, c2, pi2, lens = honest(env, [4] * 5)
    c2[1] = g2_mul(k, env.f[1] + q)
    c2[3] = g2_mul(k, env.f[3] - q)
    hdr = (c, c2, pi2, lens)
    assert reference(k, env, hdr, only=[1, 3]) is False
    assert batch(k, env, hdr, weights=_ones(5)) is True
    assert batch(k, env, hdr) is False


def test_rho_separates_the_two_equations(k, env):
    q = 0x1122334455667788
    c, c2, pi2, lens = honest(env, three_groups(7))
    i, d = 2, three_groups(7)[2]
    c2[i] = g2_mul(k, env.f[i] + q)                                 # (C, C2 + Q, pi2 + [tau^(N-d)]Q): the second equation still holds
    pi2[i] = g2_mul(k, env.shift_scalar[d] * (env.f[i] + q))
    hdr = (c, c2, pi2, lens)
    assert k.helpers.pairings_verify(env.shifts[d], c2[i], g1_mul(1), pi2[i]) is True
    assert reference(k, env, hdr, only=[i]) is False
    assert batch(k, env, hdr) is False


def test_supplied_full_width_weights(k, env):
    rnd = random.Random(77)
    count = 66
    w = [rnd.randrange(1, R_) for _ in range(count + 1)]
    w[3], w[65], w[10] = R_ - 1, R_ - 2, 0
    weights = pyref.frs_to_mont(w)
    lens = three_groups(count)
    assert batch(k, env, honest(env, lens), weights=weights) is True
    for pos in (3, 64, 65):
        c, c2, pi2, _ = honest(env, lens)
        pi2[pos] = env.pi2[4][201]
        assert batch(k, env, (c, c2, pi2, lens), weights=weights) is False, pos
        c, c2, pi2, _ = honest(env, lens)
        c2[pos] = env.c2[201]
        assert batch(k, env, (c, c2, pi2, lens), weights=weights) is False, pos
    # a weight of 0 makes its item's tampering invisible: the supplied weight is the one the kernel and the MSM use
    c, c2, pi2, _ = honest(env, lens)
    c[10], c2[10], pi2[10] = env.c[202], env.c2[203], env.pi2[1][204]
    hdr = (c, c2, pi2, lens)
    assert reference(k, env, hdr, only=[10]) is False
    assert batch(k, env, hdr, weights=weights) is True
    assert batch(k, env, hdr) is False


# ---- the subgroup test --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bad_points(env):
    rnd = random.Random(88)
    off = env.c2[7].copy(); off[1] ^= np.uint64(1)                  # off the twist
    tw = g2.to_wire(g2.random_twist_point(rnd))                     # on the twist, outside the subgroup
    small = g2.to_wire(g2.add(g2.point_of_order(10069, rnd), g2.from_wire(env.c2[8])))   # a small-order component behind a subgroup point
    return {"off": off, "twist": tw, "small": small}


def _host_first_bad(k, pts):
    for i, p in enumerate(pts):
        reason = k._lib.i32(0)
        assert k._lib.load().kzg_validate_g2_point(k._lib.ptr(np.ascontiguousarray(p)), C.byref(reason)) == 0
        if reason.value in (1, 3):                                  # not on the curve / not in the subgroup
            return i
    return None


@pytest.mark.parametrize("first", [0, 255, 256, 299, None])
def test_check_subgroup_reports_the_first_bad_point(k, env, bad_points, first):
    base = np.concatenate([env.c2[:POOL], env.pi2[4][:40]])         # 300 subgroup points
    assert len(base) == 300
    for kind, bp in bad_points.items():
        pts = base.copy()
        if first is not None:
            pts[first] = bp
            if first < 290:
                pts[first + 5] = bad_points["twist"]                # a later one does not matter
        if first is None:
            k.helpers.check_g2_subgroup(pts, ctx=env.ctx)
            break
        assert _host_first_bad(k, pts[:first + 1]) == first
        bad = C.c_uint64(2 ** 64 - 1)
        rc = k._lib.load().kzg_g2_check_subgroup(env.ctx.handle, k._lib.ptr(pts), len(pts), C.byref(bad))
        assert (rc, bad.value) == (NOT_ON_CURVE, first), kind
        with pytest.raises(k.errors.NotOnCurveError, match="point %d " % first):
            k.helpers.check_g2_subgroup(pts, ctx=env.ctx)
    pts = base.copy(); pts[100] = 0                                 # the identity passes
    k.helpers.check_g2_subgroup(pts, ctx=env.ctx)
    k.helpers.check_g2_subgroup(np.zeros((0, 16), np.uint64), ctx=env.ctx)


def test_batch_reports_the_header_of_a_point_outside_the_subgroup(k, env, bad_points):
    lens = three_groups(70)
    for kind, want in (("twist", NOT_ON_CURVE), ("small", NOT_ON_CURVE), ("off", G2_OFF)):
        for which, pos in (("c2", 64), ("pi2", 5), ("c2", 69)):
            c, c2, pi2, _ = honest(env, lens)
            (c2 if which == "c2" else pi2)[pos] = bad_points[kind]
            (pi2 if which == "c2" else c2)[69] = bad_points[kind]   # a later one (or the same header's other element)
            rc, ok, bad = raw(k, env, (c, c2, pi2, lens))
            assert (rc, bad) == (want, pos), (kind, which, pos)
    # both kinds in one batch: the on-twist rule comes first, whatever the positions
    c, c2, pi2, _ = honest(env, lens)
    c2[2] = bad_points["small"]; pi2[40] = bad_points["off"]
    assert raw(k, env, (c, c2, pi2, lens))[::2] == (G2_OFF, 40)
    with pytest.raises(k.errors.NotOnCurveError, match="header 40 not on curve"):
        batch(k, env, (c, c2, pi2, lens))
    assert batch(k, env, honest(env, lens)) is True


# ---- errors, in their order -----------------------------------------------------------------------------------------------------------
def test_every_error_in_its_order(k, env, bad_points):
    lens = three_groups(5)
    good = honest(env, lens)
    sl, sp = list(env.shifts), np.stack(list(env.shifts.values()))

    def usable():
        assert raw(k, env, good)[:2] == (OK, 1)

    off_c = good[0].copy(); off_c[3, 0] ^= np.uint64(1)
    # 1. pointers and the shape of the shift list
    for name in ("c", "c2", "pi2", "lens", "sl", "sp"):
        assert raw(k, env, good, nulls=(name,))[0] == INVALID, name
    assert raw(k, env, good, shift_lens=[], shift_pts=np.zeros((0, 8), np.uint64))[0] == INVALID
    many = [3 * (j + 1) for j in range(65)]                         # 65 shifts, none a power of two: rule 1 in front of rule 2
    assert raw(k, env, good, shift_lens=many, shift_pts=np.tile(sp[0], (65, 1)))[0] == INVALID
    assert raw(k, env, good, shift_lens=[1, 4, 1024, 4], shift_pts=np.concatenate([sp, sp[1:2]]))[0] == INVALID
    assert raw(k, env, good, shift_lens=[3, 4, 1024, 3], shift_pts=np.concatenate([sp, sp[:1]]))[0] == INVALID     # duplicate and not a power of two
    usable()
    # 2. powers of two
    assert raw(k, env, good, shift_lens=[1, 4, 1000])[0] == NOT_POW2
    assert raw(k, env, (good[0], good[1], good[2], [4, 4, 6, 4, 0]))[0] == NOT_POW2
    assert raw(k, env, (off_c, good[1], good[2], [4, 4, 6, 4, 2]))[0] == NOT_POW2        # 6 (rule 2) in front of 2 (rule 3) and the commitment (rule 5)
    usable()
    # 3. a claimed length without a shift
    assert raw(k, env, (off_c, good[1], good[2], [4, 1, 4, 2, 8]))[::2] == (INVALID, 3)
    usable()
    # 4. size (the arrays are never read beyond the lengths: untouched zero pages)
    big = (1 << 20) + 1
    zc, z2 = np.zeros((big, 8), np.uint64), np.zeros((big, 16), np.uint64)
    zc[0, 0] = 1                                                    # off the curve: rule 4 in front of rule 5
    assert raw(k, env, (zc, z2, z2, np.full(big, 4, np.uint64)))[0] == TOO_LARGE
    del zc, z2
    usable()
    # 5. G1 inputs
    off2 = good[1].copy(); off2[0] = bad_points["off"]
    assert raw(k, env, (off_c, off2, good[2], lens))[::2] == (G1_OFF, 3)                  # in front of rule 6
    bad_sp = sp.copy(); bad_sp[2, 5] ^= np.uint64(1)
    assert raw(k, env, (good[0], off2, good[2], lens), shift_pts=bad_sp)[::2] == (G1_OFF, 2)
    with pytest.raises(k.errors.NotOnCurveError, match="G1 point 3"):
        batch(k, env, (off_c, good[1], good[2], lens))
    usable()
    # 6. off the twist, 7. outside the subgroup
    out2 = good[2].copy(); out2[1] = bad_points["twist"]
    assert raw(k, env, (good[0], off2, out2, lens))[::2] == (G2_OFF, 0)
    usable()
    assert raw(k, env, (good[0], good[1], out2, lens))[::2] == (NOT_ON_CURVE, 1)
    usable()
    # a failed equation is no error
    assert raw(k, env, (good[0], good[1], np.roll(good[2], 1, axis=0), lens))[:2] == (OK, 0)
    assert sl == list(LENS)


def test_equal_inputs_on_a_second_context_give_equal_answers(k, env, bad_points):
    other = k._lib.Context(0)
    lens = three_groups(65)
    good = honest(env, lens)
    c, c2, pi2, _ = honest(env, lens)
    pi2[64] = env.pi2[4][205]
    out = good[2].copy(); out[9] = bad_points["small"]
    for hdr in (good, (c, c2, pi2, lens), (good[0], good[1], out, lens)):
        assert raw(k, env, hdr) == raw(k, env, hdr, ctx=other)
    w = k.verifier.compute_header_batch_weights(*good, env.shifts)
    assert raw(k, env, good, weights=w) == raw(k, env, good, ctx=other) == (OK, 1, 2 ** 64 - 1)
    other.close()
