"""-m gpu: locating the bad headers of a batch (`kzg_header_group_sums`, `kzg_verify_length_proof_batch_locate`).

The setting of tests/test_gpu_header_batch.py: a known tau over a setup of order N = 2^10, the lengths (1, 4, 1024), a pool of headers
C = [f]_1, C2 = [f]_2, pi2 = [tau^(N-d) f]_2 with known scalars f, made by the host's fixed-base multiplication.  With supplied weights
r_i the group sums have a closed form in those scalars,
    U_g = [sum r_i f_i]_1,   W_(g,s) = [sum_{d_i = s} r_i f_i]_2,   Pi_g = [sum r_i f_i tau^(N - d_i)]_2,
and the device's outputs must match it bit for bit.  The reference of every good / bad decision is the loop of the single-call
`kzg_verify_length_proof` over the same items."""
import ctypes as C
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import g2_points as g2
import pyref
from pyref import R_

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
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
    return k.helpers.g2_mul_generator(pyref.fr_to_mont(s % R_)) if s % R_ else np.zeros(16, np.uint64)


class Env:
    pass


@pytest.fixture(scope="module")
def env(k):
    """a pool of honest headers by their scalars: header i of length d is (c[i], c2[i], pi2[d][i]).  Computed once and never written:
    every test works on copies.  f[POOL] = -f[0] and f[POOL + 1] = 0 (the zero polynomial)."""
    e = Env()
    rnd = random.Random(2025)
    e.tau = rnd.randrange(2, R_)
    e.shift_scalar = {d: pow(e.tau, N - d, R_) for d in LENS}
    e.shifts = {d: g1_mul(s) for d, s in e.shift_scalar.items()}
    e.f = [rnd.randrange(1, R_) for _ in range(POOL)]
    e.f += [R_ - e.f[0], 0]
    e.c = np.stack([g1_mul(f) for f in e.f])
    e.c2 = np.stack([g2_mul(k, f) for f in e.f])
    e.pi2 = {d: np.stack([g2_mul(k, e.shift_scalar[d] * f) for f in e.f]) for d in LENS}
    e.ctx = k._lib.Context(0)
    return e


NEG0, ZERO = POOL, POOL + 1


def pick(env, idx, lens):
    """(commitments, length commitments, length proofs, lens) of the pool headers idx with these lengths: copies"""
    idx = list(idx)
    if not idx:
        return np.zeros((0, 8), np.uint64), np.zeros((0, 16), np.uint64), np.zeros((0, 16), np.uint64), []
    return env.c[idx].copy(), env.c2[idx].copy(), np.stack([env.pi2[d][i] for i, d in zip(idx, lens)]), list(lens)


def honest(env, lens):
    return pick(env, range(len(lens)), lens)


def three_classes(count):
    """the three lengths alternating: the segments of the sorted lanes change inside a wave"""
    return [LENS[i % 3] for i in range(count)]


def uneven(count):
    """five groups: a large one, an EMPTY one, a group of one between two large ones, a large one, an empty one at the end"""
    gi = [0 if i < count // 2 else 3 for i in range(count)]
    gi[count // 2] = 2
    return gi, 5


def weights128(seed, count):
    rnd = random.Random(seed)
    return [rnd.randrange(1, 1 << 128) for _ in range(count + 1)]


def closed_form(k, env, idx, lens, w, gi, n_groups):
    """(u, u_is_infinity, w, pi) from the scalars"""
    su = [0] * n_groups
    sp = [0] * n_groups
    sw = [[0] * len(LENS) for _ in range(n_groups)]
    for j, (i, d) in enumerate(zip(idx, lens)):
        g = gi[j]
        su[g] += w[j] * env.f[i]
        sp[g] += w[j] * env.f[i] * env.shift_scalar[d]
        sw[g][LENS.index(d)] += w[j] * env.f[i]
    u = np.stack([g1_mul(s) for s in su]) if n_groups else np.zeros((0, 8), np.uint64)
    uinf = np.array([s % R_ == 0 for s in su], bool)
    wg = np.array([[g2_mul(k, s) for s in row] for row in sw], np.uint64).reshape(n_groups, len(LENS), 16)
    pi = np.array([g2_mul(k, s) for s in sp], np.uint64).reshape(n_groups, 16)
    return u, uinf, wg, pi


def sums(k, env, hdr, w, groups, n_groups=None, ctx=None):
    c, c2, pi2, lens = hdr
    return k.verifier.header_group_sums(c, c2, pi2, lens, env.shifts, weights=None if w is None else pyref.frs_to_mont(w), ctx=ctx or env.ctx, groups=groups,
                                        n_groups=n_groups)


def same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want)) and len(got) == len(want) == 4


# ---- 1. group sums against the closed form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouping", ["item", "one", "uneven"])
@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 257])          # the wave (64) and workgroup (256) edges of 2 count lanes
def test_group_sums_are_bit_equal_to_the_closed_form(k, env, count, grouping):
    # "one": every header of ONE length in one group -- at 65 the C2 segment spans two waves and the pi2 segment starts mid-wave, the
    # smallest shape with more than one partial per segment
    lens = [4] * count if grouping == "one" else three_classes(count)
    if grouping == "item":
        gi, n_groups, arg = list(range(count)), count, "item"
    elif grouping == "one":
        gi, n_groups = [0] * count, 1
        arg = gi
    else:
        gi, n_groups = uneven(count)
        arg = gi
    w = weights128(count, count)
    got = sums(k, env, honest(env, lens), w, arg, None if arg == "item" else n_groups)
    want = closed_form(k, env, range(count), lens, w, gi, n_groups)
    assert got[0].shape == (n_groups, 8) and got[2].shape == (n_groups, 3, 16) and got[3].shape == (n_groups, 16)
    assert same(got, want)
    if grouping == "uneven":
        assert got[1][1] and got[1][4] and not got[2][1].any() and not got[3][4].any()      # the empty groups: identities


def test_full_width_weights_and_the_sum_over_all_groups(k, env):
    """254-bit weights (the chains run over the largest), and the components summed over the groups are those of one group"""
    rnd = random.Random(9)
    count = 66
    w = [rnd.randrange(1, R_) for _ in range(count + 1)]
    w[3], w[10] = R_ - 1, 0
    lens = three_classes(count)
    gi, n_groups = uneven(count)
    got = sums(k, env, honest(env, lens), w, gi, n_groups)
    assert same(got, closed_form(k, env, range(count), lens, w, gi, n_groups))
    assert same(sums(k, env, honest(env, lens), w, [0] * count, 1), closed_form(k, env, range(count), lens, w, [0] * count, 1))


# ---- 2. exceptional additions inside one segment --------------------------------------------------------------------------------------------
def test_exceptional_additions_inside_a_segment(k, env):
    """Equal supplied weights: the same header twice (the doubling path of the first scan step), a header beside the header of r - f
    (the sum is the identity), the zero header, a group of nothing but identities"""
    idx = [0, 0,          # group 0: P + P
           1, 1, 1,       # group 1: P + P, then 2P + P
           0, NEG0,       # group 2: P + (-P)
           2, ZERO,       # group 3: the zero header beside an honest one
           ZERO, ZERO, ZERO,   # group 4: nothing but identities
           NEG0, 0, 0, NEG0, 3]   # group 5: cancellations inside a longer run
    gi = [0, 0, 1, 1, 1, 2, 2, 3, 3, 4, 4, 4, 5, 5, 5, 5, 5]
    lens = [4] * len(idx)
    for r in (1, 0xFEDCBA9876543210FEDCBA9876543211):
        w = [r] * len(idx) + [7]
        got = sums(k, env, pick(env, idx, lens), w, gi, 6)
        assert same(got, closed_form(k, env, idx, lens, w, gi, 6)), r
        assert got[1][2] and got[1][4] and not got[2][2].any() and not got[3][2].any() and not got[2][4].any() and not got[3][4].any()
        assert not got[1][0] and got[2][0, 1].any() and not got[2][0, 0].any()
    # the same across two waves: 40 copies of one header, then 40 of its negation, in one group
    idx = [0] * 40 + [NEG0] * 40 + [5]
    w = [3] * len(idx) + [1]
    got = sums(k, env, pick(env, idx, [1] * len(idx)), w, [0] * len(idx), 1)
    assert same(got, closed_form(k, env, idx, [1] * len(idx), w, [0] * len(idx), 1))
    # ... and the search on such a batch: every header is honest
    c, c2, pi2, lens = pick(env, idx, [1] * len(idx))
    good, checks = k.verifier.locate_bad_headers(c, c2, pi2, lens, env.shifts, weights=pyref.frs_to_mont(w), ctx=env.ctx, groups="item")
    assert good.all() and checks == 1


# ---- 3. permutation invariance -----------------------------------------------------------------------------------------------------------
def test_permuting_the_headers_inside_groups_changes_no_bit(k, env):
    count = 130
    lens = three_classes(count)
    gi = [(i * 7) % 4 for i in range(count)]
    w = weights128(3, count)
    base = sums(k, env, honest(env, lens), w, gi, 4)
    perm = list(range(count))
    random.Random(4).shuffle(perm)
    got = sums(k, env, pick(env, perm, [lens[i] for i in perm]), [w[i] for i in perm] + [w[count]], [gi[i] for i in perm], 4)
    assert same(got, base)
    other = k._lib.Context(0)                                        # ... and neither does another context
    assert same(sums(k, env, honest(env, lens), w, gi, 4, ctx=other), base)
    other.close()


# ---- 4. locate against the loop of verify_length_proof ---------------------------------------------------------------------------------------
def bound(n_groups, b):
    return 1 + 2 * b * math.ceil(math.log2(n_groups)) if n_groups > 1 else 1


def reference_groups(k, env, hdr, gi, n_groups, only):
    """per group: all(kzg_verify_length_proof(header)); `only`: the headers that differ from the pool's honest ones (the others are known)"""
    c, c2, pi2, lens = hdr
    good = np.ones(n_groups, bool)
    for i in only:
        if not k.verifier.verify_length_proof(c[i], c2[i], pi2[i], env.shifts[lens[i]]):
            good[gi[i]] = False
    return good


def locate(k, env, hdr, groups="item", n_groups=None, weights=None, only=()):
    """locate_bad_headers, checked against the reference loop, the bound on the checks and the batch entry's verdict"""
    c, c2, pi2, lens = hdr
    count = len(lens)
    gi = list(range(count)) if isinstance(groups, str) else list(groups)
    G = count if isinstance(groups, str) else n_groups
    good, checks = k.verifier.locate_bad_headers(c, c2, pi2, lens, env.shifts, weights=weights, ctx=env.ctx, groups=groups, n_groups=n_groups)
    want = reference_groups(k, env, hdr, gi, G, only)
    assert good.shape == (G,) and list(good) == list(want), (np.flatnonzero(~good), np.flatnonzero(~want))
    b = int((~good).sum())
    assert checks <= bound(G, b), (checks, G, b)
    if b == 0:
        assert checks == (1 if count else 0)
    assert bool(good.all()) is k.verifier.verify_length_proof_batch(c, c2, pi2, lens, env.shifts, weights=weights, ctx=env.ctx)
    return good, checks


def tamper(env, hdr, pos, what, other=200):
    c, c2, pi2, lens = hdr
    if what == "C":
        c[pos] = env.c[other]
    elif what == "C2":
        c2[pos] = env.c2[other]
    elif what == "pi2":
        pi2[pos] = env.pi2[lens[pos]][other]
    else:
        lens[pos] = 1 if lens[pos] != 1 else 4                       # another listed length: the proof is for the first


@pytest.mark.parametrize("count", [1, 65, 257])
def test_an_honest_batch_is_all_good_with_one_check(k, env, count):
    hdr = honest(env, three_classes(count))
    good, checks = locate(k, env, hdr)
    assert good.all() and checks == 1
    gi, G = uneven(count)
    good, checks = locate(k, env, hdr, groups=gi, n_groups=G)
    assert good.all() and checks == 1
    good, checks = locate(k, env, hdr, weights=pyref.frs_to_mont(weights128(1, count)))
    assert good.all() and checks == 1


@pytest.mark.parametrize("pos", [0, 63, 64])                        # 64 is the last of 65
@pytest.mark.parametrize("what", ["C", "C2", "pi2", "d"])
def test_one_bad_header_marks_exactly_its_group(k, env, pos, what):
    hdr = honest(env, [4] * 65)
    tamper(env, hdr, pos, what)
    good, checks = locate(k, env, hdr, only=[pos])
    assert list(np.flatnonzero(~good)) == [pos] and checks <= 1 + 2 * 7


def test_three_bad_headers_in_257(k, env):
    lens = three_classes(257)
    hdr = honest(env, lens)
    for pos, what in ((100, "pi2"), (101, "C2"), (256, "C")):       # two adjacent
        tamper(env, hdr, pos, what, other=201 + pos % 3)
    good, checks = locate(k, env, hdr, only=[100, 101, 256])
    assert list(np.flatnonzero(~good)) == [100, 101, 256]
    gi = [i // 30 for i in range(257)]                               # 9 groups: 100 and 101 share group 3, 256 is alone in group 8
    good, checks = locate(k, env, hdr, groups=gi, n_groups=9, only=[100, 101, 256])
    assert list(np.flatnonzero(~good)) == [3, 8]
    good, checks = locate(k, env, hdr, groups=gi, n_groups=9, only=[100, 101, 256], weights=pyref.frs_to_mont(weights128(8, 257)))
    assert list(np.flatnonzero(~good)) == [3, 8]


def test_all_headers_bad(k, env):
    c, c2, pi2, lens = honest(env, [4] * 9)
    hdr = (c, c2, np.roll(pi2, 1, axis=0), lens)
    good, checks = locate(k, env, hdr, only=range(9))
    assert not good.any()
    good, checks = locate(k, env, hdr, groups=[0, 0, 0, 1, 1, 1, 2, 2, 2], n_groups=3, only=range(9))
    assert not good.any()


def test_the_trace_names_the_phases():
    """KZG_VB_TRACE is read when the library loads: a child process"""
    body = r'''
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import torch  # noqa: F401  (load order: tests/conftest.py)
import numpy as np
import rust_kzg_bn254_amd as k
import pyref
g1 = pyref.point_to_wire((1, 2))
z = np.zeros((3, 16), np.uint64)
good, checks = k.verifier.locate_bad_headers(np.stack([g1] * 3), z, z, [4, 4, 4], {4: g1})
print("RESULT", [bool(g) for g in good], checks)
''' % {"root": ROOT}
    res = subprocess.run([sys.executable, "-c", body], capture_output=True, text=True, timeout=300, env=dict(os.environ, KZG_VB_TRACE="1"), cwd=ROOT)
    assert res.returncode == 0 and "RESULT [False, False, False] " in res.stdout, (res.stdout[-2000:], res.stderr[-2000:])
    line = [ln for ln in res.stderr.splitlines() if "verify_length_proof_batch_locate" in ln]
    assert len(line) == 1, res.stderr[-2000:]
    for phase in ("shared prefix", "G2 group sums", "G1 group sums", "host sums", "search", "pairing checks", "3 bad groups"):
        assert phase in line[0], line[0]


# ---- 5. the error table, in its order -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bad_points(env):
    rnd = random.Random(88)
    off = env.c2[7].copy(); off[1] ^= np.uint64(1)                  # off the twist
    tw = g2.to_wire(g2.random_twist_point(rnd))                     # on the twist, outside the subgroup
    return {"off": off, "twist": tw}


def raw(k, env, hdr, entry="locate", gi=None, n_groups=None, shift_lens=None, shift_pts=None, nulls=(), count=None, weights=None):
    """the C-ABI calls themselves: (status, bad_index, outputs)"""
    L = k._lib
    c, c2, pi2, lens = hdr
    c = np.ascontiguousarray(c, np.uint64); c2 = np.ascontiguousarray(c2, np.uint64); pi2 = np.ascontiguousarray(pi2, np.uint64)
    lens = np.ascontiguousarray(lens, np.uint64)
    n = len(lens) if count is None else count
    gi = np.ascontiguousarray(np.arange(n) if gi is None else gi, np.uint64)
    G = n if n_groups is None else n_groups
    sl = np.ascontiguousarray(list(env.shifts) if shift_lens is None else shift_lens, np.uint64)
    sp = np.ascontiguousarray(np.stack(list(env.shifts.values())) if shift_pts is None else shift_pts, np.uint64)
    opt = lambda a: L.ptr(a) if a.size else None                    # noqa: E731
    args = {"c": opt(c), "c2": opt(c2), "pi2": opt(pi2), "lens": opt(lens), "sl": opt(sl), "sp": opt(sp), "gi": opt(gi)}
    out_n = max(min(G, 1 << 12), 1)                                 # (a refused n_groups writes nothing)
    o = {"ok": np.full(out_n, 7, np.uint8), "u": np.full((out_n, 8), 7, np.uint64), "uinf": np.full(out_n, 7, np.uint8),
         "w": np.full((out_n, max(len(sl), 1), 16), 7, np.uint64), "pi": np.full((out_n, 16), 7, np.uint64)}
    n_bad, checks, bad = L.sz(77), L.sz(77), C.c_uint64(2 ** 64 - 1)
    u8 = lambda a: a.ctypes.data_as(L.u8p)                          # noqa: E731
    outs = {"ok": u8(o["ok"]), "n_bad": C.byref(n_bad), "u": L.ptr(o["u"]), "uinf": u8(o["uinf"]), "w": L.ptr(o["w"]), "pi": L.ptr(o["pi"])}
    for name in nulls:
        (args if name in args else outs)[name] = None
    w = None if weights is None else L.ptr(np.ascontiguousarray(weights, np.uint64))
    head = (env.ctx.handle, args["c"], args["c2"], args["pi2"], args["lens"], n, args["sl"], args["sp"], len(sl), w, args["gi"], G)
    if entry == "locate":
        rc = L.load().kzg_verify_length_proof_batch_locate(*head, outs["ok"], outs["n_bad"], C.byref(checks), C.byref(bad))
    else:
        rc = L.load().kzg_header_group_sums(*head, outs["u"], outs["uinf"], outs["w"], outs["pi"], C.byref(bad))
    o["n_bad"], o["checks"] = n_bad.value, checks.value
    return rc, bad.value, o


def untouched(o):
    return (o["ok"] == 7).all() and (o["u"] == 7).all() and (o["uinf"] == 7).all() and (o["w"] == 7).all() and (o["pi"] == 7).all() and o["n_bad"] == 77 and o["checks"] == 77


@pytest.mark.parametrize("entry", ["locate", "sums"])
def test_every_error_in_its_order(k, env, bad_points, entry):
    lens = [4, 1, 4, 1024, 1]
    good = honest(env, lens)
    sp = np.stack(list(env.shifts.values()))

    def usable():
        rc, bad, o = raw(k, env, good, entry)
        assert rc == OK and (entry == "sums" or (o["n_bad"], o["checks"], list(o["ok"][:5])) == (0, 1, [1] * 5))

    def refused(want, want_bad=2 ** 64 - 1, **kw):
        rc, bad, o = raw(k, env, kw.pop("hdr", good), entry, **kw)
        assert (rc, bad) == (want, want_bad) and untouched(o), (rc, bad, kw)

    off_c = good[0].copy(); off_c[3, 0] ^= np.uint64(1)
    off2 = good[1].copy(); off2[0] = bad_points["off"]
    # 1. pointers (group_indices and the outputs among them) and the shape of the shift list -- in front of every later row
    later = dict(hdr=(off_c, off2, good[2], [4, 6, 4, 2, 1]), gi=[0, 1, 9, 3, 4])
    for name in ("c", "c2", "pi2", "lens", "sl", "sp", "gi") + (("ok", "n_bad") if entry == "locate" else ("u", "uinf", "w", "pi")):
        refused(INVALID, nulls=(name,), **later)
    refused(INVALID, shift_lens=[], shift_pts=np.zeros((0, 8), np.uint64), **later)
    refused(INVALID, shift_lens=[1, 4, 1024, 4], shift_pts=np.concatenate([sp, sp[1:2]]), **later)
    usable()
    # 2. powers of two, in front of 3, 4a and 5
    refused(NOT_POW2, **later)
    refused(NOT_POW2, shift_lens=[1, 4, 1000], gi=[0, 1, 9, 3, 4])
    # 3. a claimed length without a shift, in front of 4a and 5
    refused(INVALID, 3, hdr=(off_c, off2, good[2], [4, 1, 4, 2, 1]), gi=[0, 1, 9, 3, 4])
    # 4. size, in front of 4a (the arrays are never read beyond the lengths: untouched zero pages)
    big = (1 << 20) + 1
    zc, z2 = np.zeros((big, 8), np.uint64), np.zeros((big, 16), np.uint64)
    zc[0, 0] = 1
    refused(TOO_LARGE, hdr=(zc, z2, z2, np.full(big, 4, np.uint64)), gi=np.full(big, 5, np.uint64), n_groups=3)
    del zc, z2
    usable()
    # 4a. the group indices, in front of 4b and of every curve check
    refused(INVALID, hdr=(off_c, off2, good[2], lens), gi=[0, 1, 5, 3, 4])                  # 5 >= n_groups = 5
    refused(INVALID, hdr=(off_c, off2, good[2], lens), gi=[0, 0, 0, 0, 0], n_groups=0)      # n_groups = 0 with count > 0
    refused(INVALID, hdr=(off_c, off2, good[2], lens), gi=[0, 0, (1 << 28), 0, 0], n_groups=1 << 28)
    # 4b. n_groups (n_shifts + 1) > 2^28, before anything of that size is allocated and in front of the curve checks; whatever the count
    refused(TOO_LARGE, hdr=(off_c, off2, good[2], lens), gi=[0, 1, 2, 3, 4], n_groups=(1 << 26) + 1)
    rc, bad, o = raw(k, env, honest(env, []), entry, n_groups=(1 << 26) + 1)
    assert rc == TOO_LARGE and untouched(o)
    usable()
    # 5. G1 inputs: the commitments, then the shifts
    refused(G1_OFF, 3, hdr=(off_c, off2, good[2], lens))                                  # in front of row 6
    bad_sp = sp.copy(); bad_sp[2, 5] ^= np.uint64(1)
    refused(G1_OFF, 2, hdr=(good[0], off2, good[2], lens), shift_pts=bad_sp)
    usable()
    # 6. off the twist, 7. outside the subgroup: the smallest header, C2 in front of pi2, 6 in front of 7 whatever the positions
    out2 = good[2].copy(); out2[1] = bad_points["twist"]
    refused(G2_OFF, 0, hdr=(good[0], off2, out2, lens))
    both = good[1].copy(); both[2] = bad_points["off"]; both[4] = bad_points["off"]
    refused(G2_OFF, 2, hdr=(good[0], both, out2, lens))
    usable()
    out1 = good[1].copy(); out1[3] = bad_points["twist"]
    refused(NOT_ON_CURVE, 1, hdr=(good[0], out1, out2, lens))
    refused(NOT_ON_CURVE, 3, hdr=(good[0], out1, good[2], lens))
    with pytest.raises(k.errors.NotOnCurveError, match="header 3 not in correct subgroup"):
        k.verifier.locate_bad_headers(good[0], out1, good[2], lens, env.shifts, ctx=env.ctx)
    with pytest.raises(k.errors.NotOnCurveError, match="G1 point 3"):
        k.verifier.header_group_sums(off_c, good[1], good[2], lens, env.shifts, ctx=env.ctx)
    with pytest.raises(k.errors.GenericError, match="group index"):
        k.verifier.locate_bad_headers(*good, env.shifts, ctx=env.ctx, groups=[0, 1, 2, 3, 4], n_groups=4)
    usable()
    # count = 0: every group good, no pairing check; identities everywhere
    rc, bad, o = raw(k, env, honest(env, []), entry, n_groups=6)
    assert rc == OK
    if entry == "locate":
        assert (o["ok"][:6] == 1).all() and (o["n_bad"], o["checks"]) == (0, 0)
        good_v, n_checks = k.verifier.locate_bad_headers(*honest(env, []), env.shifts, ctx=env.ctx, groups=[], n_groups=4)
        assert good_v.shape == (4,) and good_v.all() and n_checks == 0
    else:
        assert not o["u"][:6].any() and (o["uinf"][:6] == 1).all() and not o["w"][:6].any() and not o["pi"][:6].any()
    # a failed equation is no error, and the context is usable after all of the above
    rc, bad, o = raw(k, env, (good[0], good[1], np.roll(good[2], 1, axis=0), lens), entry)
    assert rc == OK and (entry == "sums" or (o["n_bad"] == 5 and not o["ok"][:5].any()))
    usable()


# ---- 6. the bound-checked build: the 65-header case with every site counter at 0 ----------------------------------------------------------------
VARIANT = os.path.join(ROOT, "rust-kzg-bn254_amd", "libkzg_bn254_mi355x_boundcheck.so")
N_SITES = 14
CHILD = r'''
import ctypes as C, os, random, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import torch  # noqa: F401  (load order: tests/conftest.py)
import numpy as np
import rust_kzg_bn254_amd as k
import pyref
from pyref import R_
L = k._lib
assert L.LIB_PATH == os.environ["KZG_LIB_PATH"], L.LIB_PATH
h = L.load()
n = h.kzg_bc_sites()
assert n == %(sites)d, n
assert h.kzg_bc_reset_all() == 0
rnd = random.Random(5)
N, tau = 1024, rnd.randrange(2, R_)
g1 = lambda s: pyref.point_to_wire(pyref.ec_mul(s %% R_, (1, 2)))
g2 = lambda s: k.helpers.g2_mul_generator(pyref.fr_to_mont(s %% R_))
lens = [4] * 65                                 # one length, one group: the C2 segment spans two waves, the pi2 segment starts mid-wave
fs = [rnd.randrange(1, R_) for _ in lens]
fs[7] = fs[6]                                   # P + P in the first scan step
shifts = {d: g1(pow(tau, N - d, R_)) for d in (1, 4, 1024)}
c = np.stack([g1(f) for f in fs]); c2 = np.stack([g2(f) for f in fs])
pi2 = np.stack([g2(pow(tau, N - d, R_) * f) for f, d in zip(fs, lens)])
w = [rnd.randrange(1, 1 << 128) for _ in range(66)]
w[7] = w[6]
u, uinf, wg, pi = k.verifier.header_group_sums(c, c2, pi2, lens, shifts, weights=pyref.frs_to_mont(w), groups=[0] * 65, n_groups=1)
s = sum(a * b for a, b in zip(w, fs))
closed = np.array_equal(u[0], g1(s)) and np.array_equal(wg[0, 1], g2(s)) and np.array_equal(pi[0], g2(s * pow(tau, N - 4, R_))) and not wg[0, 0].any()
good, checks = k.verifier.locate_bad_headers(c, c2, pi2, lens, shifts)                       # derived weights, one group per header
pi2[64] = pi2[63]
full = pyref.frs_to_mont([rnd.randrange(R_) for _ in range(66)])                             # 254-bit chains
bad, checks2 = k.verifier.locate_bad_headers(c, c2, pi2, lens, shifts, weights=full, groups=[i // 8 for i in range(65)], n_groups=9)
counts = (C.c_ulonglong * n)(); first = (C.c_int32 * (9 * n))()
assert h.kzg_bc_read_all(counts, first) == 0
print("RESULT", int(closed), int(good.all()), checks, [int(g) for g in np.flatnonzero(~bad)])
for s in range(n):
    print("SITE", s, counts[s], *first[9 * s:9 * s + 9])
'''


def test_the_locate_kernels_stay_inside_every_precondition():
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    body = CHILD % {"root": ROOT, "sites": N_SITES}
    res = subprocess.run([sys.executable, "-c", body], capture_output=True, text=True, timeout=300, env=dict(os.environ, KZG_LIB_PATH=VARIANT), cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "RESULT 1 1 1 [8]" in out, (out[-3000:], res.stderr[-2000:])
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert len(sites) == N_SITES
    fired = [(int(s[1]), int(s[2]), s[3:]) for s in sites if int(s[2]) != 0]
    assert not fired, "bound violations on the device (site, count, first operand limbs): %r" % (fired,)
