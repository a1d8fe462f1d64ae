"""-m gpu: locating the bad groups of a batch of coset proofs (`kzg_coset_group_sums`, `kzg_verify_multiproof_batch_locate`): the group
sums bit-equal to big integers for every grouping that puts a segment edge somewhere else, independence of the item order, agreement of
the summed groups with `verify_multiproof_batch` on both transcript paths, the located set and the number of pairing checks for planted
corruptions, the error table, and the bound-checked build.  The world is that of tests/test_gpu_multiproof_verify.py: an SRS generated
from a known tau, random polynomials of 4 096 evaluations, proofs from `compute_multiproofs`.

The reference of the sums: per item, with python integers and the group law on the points the call is given,
    L_i = [r_i] pi_i,   R_i = [r_i] C_{c_i} + [r_i w^(k_i l)] pi_i - [r_i I_i(tau)] G1
(I_i from tests/coset_ref.py; sum_t a_t [tau^t]_1 = [I_i(tau)] G1 because the SRS is [tau^t] G1 by construction), added per group and
brought to affine coordinates: every word of every output must match."""
import ctypes as C
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import coset_ref
import pyref
from pyref import P, R_

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TAU = int.from_bytes(__import__("hashlib").sha256(b"kzg-bn254-mi355x/multiproof-locate/v1").digest(), "big") % R_
N_DOMAIN = 4096
G1 = (1, 2)


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


def rand_ints(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R_) for _ in range(n)]


# ---- the group law in Jacobian coordinates (python ints; None = identity): the affine law of pyref costs one inversion per addition ----
def jac(p):
    return None if p is None else (p[0], p[1], 1)


def jdbl(a):
    if a is None or a[1] == 0:
        return None
    x, y, z = a
    s = 4 * x * y * y % P
    m = 3 * x * x % P
    x3 = (m * m - 2 * s) % P
    return (x3, (m * (s - x3) - 8 * pow(y, 4, P)) % P, 2 * y * z % P)


def jadd(a, b):
    if a is None:
        return b
    if b is None:
        return a
    x1, y1, z1 = a
    x2, y2, z2 = b
    z1z1, z2z2 = z1 * z1 % P, z2 * z2 % P
    u1, u2 = x1 * z2z2 % P, x2 * z1z1 % P
    s1, s2 = y1 * z2 * z2z2 % P, y2 * z1 * z1z1 % P
    if u1 == u2:
        return jdbl(a) if s1 == s2 else None
    h, r = (u2 - u1) % P, (s2 - s1) % P
    hh = h * h % P
    hhh, v = h * hh % P, u1 * hh % P
    x3 = (r * r - hhh - 2 * v) % P
    return (x3, (r * (v - x3) - s1 * hhh) % P, z1 * z2 * h % P)


def jmul(kk, p):
    kk %= R_
    acc, base = None, jac(p)
    while kk:
        if kk & 1:
            acc = jadd(acc, base)
        base = jdbl(base)
        kk >>= 1
    return acc


def jneg(a):
    return None if a is None else (a[0], (-a[1]) % P, a[2])


def jaffine(a):
    if a is None:
        return None
    zi = pow(a[2], -1, P)
    return (a[0] * zi * zi % P, a[1] * zi * zi * zi % P)


def test_jacobian_helpers_are_the_affine_law():
    rnd = random.Random(5)
    p, q = pyref.ec_mul(rnd.randrange(R_), G1), pyref.ec_mul(rnd.randrange(R_), G1)
    assert jaffine(jadd(jac(p), jac(q))) == pyref.ec_add(p, q)
    assert jaffine(jadd(jac(p), jac(p))) == pyref.ec_add(p, p) and jadd(jac(p), jneg(jac(p))) is None
    s = rnd.randrange(R_)
    assert jaffine(jmul(s, p)) == pyref.ec_mul(s, p) and jmul(0, p) is None and jmul(s, None) is None


class World:
    """`n_polys` random polynomials of 4 096 evaluations on a known-tau SRS (plus, from row n_polys on, a constant polynomial -- identity
    proofs -- and the zero polynomial -- identity commitment too); per chunk length their proofs and cosets."""

    def __init__(self, k, n_polys):
        self.k, self.n = k, N_DOMAIN
        self.srs = k.SRS.generate(TAU, self.n)
        self.kz = k.KZG.new()
        self.kz.calculate_and_store_roots_of_unity(self.n * 32)
        self.polys = [k.PolynomialEvalForm(pyref.frs_to_mont(rand_ints(self.n, 1900 + i))) for i in range(n_polys)]
        self.polys.append(k.PolynomialEvalForm(pyref.frs_to_mont([777] * self.n)))
        self.polys.append(k.PolynomialEvalForm(np.zeros((self.n, 4), np.uint64)))
        self.commitments = [self.kz.commit_eval_form(p, self.srs) for p in self.polys]
        self._by_l = {}

    def at(self, l):
        if l not in self._by_l:
            proofs = [self.kz.compute_multiproofs(p, self.srs, l) for p in self.polys]
            cosets = [self.kz.cosets(p, l) for p in self.polys]
            g2 = self.k.helpers.g2_mul_generator(self.k.fr.fr_from_int(pow(TAU, l, R_)))
            self._by_l[l] = (proofs, cosets, g2)
        return self._by_l[l]

    def items(self, l, rows, ks):
        proofs, cosets, g2 = self.at(l)
        ys = np.ascontiguousarray(np.stack([cosets[c][kk] for c, kk in zip(rows, ks)]))
        pf = [proofs[c][kk] for c, kk in zip(rows, ks)]
        return ys, pf, g2


@pytest.fixture(scope="module")
def world(k):
    return World(k, 3)


@pytest.fixture(scope="module")
def world8(k):
    return World(k, 8)


# ---- 1. group sums against big integers ---------------------------------------------------------------------------------------------
def item_terms(commitments, rows, ks, ys, proofs, weights, n):
    """Per item the Jacobian pair (L_i, R_i) of the module docstring."""
    l = ys.shape[1]
    w = pyref.root_of_unity(n.bit_length() - 1)
    cm = [pyref.point_from_wire(c) for c in commitments]
    out = []
    for i, (c, kk, r) in enumerate(zip(rows, ks, weights)):
        pi = pyref.point_from_wire(proofs[i])
        coeffs = coset_ref.interpolation_coeffs(pyref.frs_from_mont(ys[i]), kk, n)
        i_tau = pyref.poly_eval(coeffs, TAU)
        right = jadd(jmul(r, cm[c]), jmul(r * pow(w, kk * l, R_), pi))
        out.append((jmul(r, pi), jadd(right, jmul(-r * i_tau, G1))))
    return out


def group_reference(terms, groups, n_groups):
    lhs, rhs = [None] * n_groups, [None] * n_groups
    for (a, b), g in zip(terms, groups):
        lhs[g], rhs[g] = jadd(lhs[g], a), jadd(rhs[g], b)
    return [jaffine(p) for p in lhs], [jaffine(p) for p in rhs]


def assert_sums(got, want, what):
    lhs, linf, rhs, rinf = got
    for side, (pts, inf, ref) in enumerate(((lhs, linf, want[0]), (rhs, rinf, want[1]))):
        assert len(pts) == len(inf) == len(ref)
        assert np.array_equal(np.asarray(pts), pyref.points_to_wire(ref)), (what, side)
        assert list(inf) == [p is None for p in ref], (what, side)


def groupings(count, rows, n_rows):
    """(name, group index per item, n_groups): every shape of segment the issue lists"""
    out = [("item", list(range(count)), count), ("all", [0] * count, 1), ("commitment", list(rows), n_rows),
           ("five with 0, 2, 4 empty", [1 + 2 * (i % 2) for i in range(count)], 5)]
    if count > 256:
        # caller order = sorted order here, so the segments end exactly at the wave edge 63|64 and the workgroup edge 255|256 ...
        out.append(("edges", [0 if i < 64 else 1 if i < 256 else 2 for i in range(count)], 3))
        # ... and here one segment crosses both
        out.append(("crossing", [0 if i < 10 else 1 if i < count - 5 else 2 for i in range(count)], 3))
    return out


def _case(world, l, count, seed):
    n, m = world.n, world.n // l
    rnd = random.Random(seed)
    rows = [i % 3 for i in range(count)]                                        # interleaved across the rows in caller order
    ks = [rnd.randrange(m) for _ in range(count)]
    weights = [rnd.randrange(R_) for _ in range(count)]
    ys, pf, _ = world.items(l, rows, ks)
    return rows, ks, weights, ys, pf


@pytest.mark.parametrize("l,count", [(l, c) for l in (1, 16, 64) for c in (1, 3, 65, 257, 600)] + [(2048, 3)])
def test_group_sums_are_bit_equal_to_big_integers(k, world, l, count):
    """3 commitments, weights supplied.  l = 2048 takes the long-coset path (one transform per coset)."""
    rows, ks, weights, ys, pf = _case(world, l, count, 31 * l + count)
    cm = world.commitments[:3]
    terms = item_terms(cm, rows, ks, ys, pf, weights, world.n)
    rp = pyref.frs_to_mont(weights)
    for name, groups, n_groups in groupings(count, rows, 3):
        got = k.verifier.coset_group_sums(cm, rows, ks, ys, pf, world.n, world.srs, rp, groups=groups, n_groups=n_groups)
        assert_sums(got, group_reference(terms, groups, n_groups), (l, count, name))
    got = k.verifier.coset_group_sums(cm, rows, ks, ys, pf, world.n, world.srs, rp, groups="commitment")       # the named groupings
    assert_sums(got, group_reference(terms, rows, 3), "commitment")
    got = k.verifier.coset_group_sums(cm, rows, ks, ys, pf, world.n, world.srs, rp, groups="item")
    assert_sums(got, group_reference(terms, list(range(count)), count), "item")


def test_group_sums_exceptional_cases_of_the_group_law(k, world):
    """l = 16.  In one call: the same item twice in a group; the same item with weights r and -r (P + (-P) inside a segment: both sums
    the identity); two equal items with equal weights (P + P); an identity proof (constant polynomial) and an identity commitment with
    an identity proof (zero polynomial); a zero weight."""
    l, n = 16, world.n
    rnd = random.Random(99)
    r = [rnd.randrange(1, R_) for _ in range(8)]
    #        twice      | r and -r         | P + P      | const | zero | zero weight
    rows = [0, 0, 1,      1, 1,              2, 2,        3,      4,     2]
    ks = [5, 5, 9,        7, 7,              11, 11,      3,      4,     8]
    weights = [r[0], r[1], r[2], r[3], R_ - r[3], r[4], r[4], r[5], r[6], 0]
    groups = [0, 0, 0,    1, 1,              2, 2,        3,      3,     4]
    ys, pf, _ = world.items(l, rows, ks)
    assert not np.asarray(pf[7]).any() and not np.asarray(pf[8]).any() and not world.commitments[4].any() and world.commitments[3].any()
    terms = item_terms(world.commitments, rows, ks, ys, pf, weights, n)
    want = group_reference(terms, groups, 5)
    assert want[0][1] is None and want[1][1] is None and want[0][3] is None and want[0][4] is None and want[1][4] is None
    got = k.verifier.coset_group_sums(world.commitments, rows, ks, ys, pf, n, world.srs, pyref.frs_to_mont(weights), groups=groups, n_groups=5)
    assert_sums(got, want, "exceptional")
    # ... and as one group each, so that P + P and P + (-P) meet at every distance of the shuffle tree
    for reps in (2, 64, 65):
        rows2, ks2 = [2] * (2 * reps), [11] * (2 * reps)
        ys2, pf2, _ = world.items(l, rows2, ks2)
        w2 = [r[4], R_ - r[4]] * reps
        got = k.verifier.coset_group_sums(world.commitments, rows2, ks2, ys2, pf2, n, world.srs, pyref.frs_to_mont(w2), groups=[0] * (2 * reps), n_groups=1)
        assert not got[0].any() and not got[2].any() and got[1][0] and got[3][0], reps
        w3 = [r[4]] * (2 * reps)
        t = item_terms(world.commitments, rows2[:1], ks2[:1], ys2[:1], pf2[:1], [2 * reps * r[4] % R_], n)
        got = k.verifier.coset_group_sums(world.commitments, rows2, ks2, ys2, pf2, n, world.srs, pyref.frs_to_mont(w3), groups=[0] * (2 * reps), n_groups=1)
        assert_sums(got, group_reference(t, [0], 1), ("equal items", reps))


# ---- 2. order independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l,count", [(16, 600), (64, 257), (2048, 3)])
def test_item_order_does_not_change_a_bit(k, world, l, count):
    rows, ks, weights, ys, pf = _case(world, l, count, 77 * l + count)
    cm = world.commitments[:3]
    rp = pyref.frs_to_mont(weights)
    for name, groups, n_groups in groupings(count, rows, 3)[2:]:
        want = k.verifier.coset_group_sums(cm, rows, ks, ys, pf, world.n, world.srs, rp, groups=groups, n_groups=n_groups)
        perm = list(range(count))
        random.Random(count).shuffle(perm)
        got = k.verifier.coset_group_sums(cm, [rows[i] for i in perm], [ks[i] for i in perm], np.ascontiguousarray(ys[perm]), [pf[i] for i in perm],
                                          world.n, world.srs, rp[perm], groups=[groups[i] for i in perm], n_groups=n_groups)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), (l, count, name)


# ---- 3. consistency with the batch entry ----------------------------------------------------------------------------------------------
def _sum_points(pts):
    acc = None
    for p in pts:
        acc = jadd(acc, jac(pyref.point_from_wire(p)))
    return pyref.point_to_wire(jaffine(acc))


@pytest.mark.parametrize("mode", [1, 2], ids=["host transcript", "device transcript"])
def test_summed_groups_agree_with_the_batch_entry(k, world, mode):
    """Weights derived (r_powers = None).  e(sum_g L_g, [tau^l]_2) = e(sum_g R_g, G2) must be `verify_multiproof_batch`'s verdict, on a
    good batch and on a corrupted one."""
    l, count = 16, 200
    rows, ks, _, ys, pf = _case(world, l, count, 4242)
    g2 = world.at(l)[2]
    cm = world.commitments[:3]
    ctx = world.srs.ctx
    V, H = k.verifier, k.helpers
    ctx.set_transcript_device(mode)
    try:
        bad = ys.copy()
        bad[123, 3] = k.fr.fr_from_int(k.fr.fr_to_int(bad[123, 3]) + 1)
        for values, expect in ((ys, True), (bad, False)):
            assert V.verify_multiproof_batch(cm, rows, ks, values, pf, world.n, world.srs, g2) is expect
            for groups, n_groups in ((rows, 3), (list(range(count)), count)):
                lhs, _, rhs, _ = V.coset_group_sums(cm, rows, ks, values, pf, world.n, world.srs, None, groups=groups, n_groups=n_groups)
                assert V.pairings_verify(_sum_points(lhs), g2, _sum_points(rhs), H.g2_generator()) is expect
            # derived weights are those of the transcript entry: supplying them changes no bit
            rp = V.compute_multiproof_r_powers(cm, rows, ks, values, pf, world.n)
            a = V.coset_group_sums(cm, rows, ks, values, pf, world.n, world.srs, None)
            b = V.coset_group_sums(cm, rows, ks, values, pf, world.n, world.srs, rp)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    finally:
        ctx.set_transcript_device(0)


# ---- 4. locate --------------------------------------------------------------------------------------------------------------------------
def _bound(n_groups, bad):
    return 1 + 2 * bad * math.ceil(math.log2(n_groups)) if n_groups > 1 else 1


@pytest.fixture(scope="module")
def batch8(world8):
    """8 commitments x 32 items, l = 16, items interleaved across the rows"""
    l = 16
    m = world8.n // l
    rnd = random.Random(808)
    rows = [i % 8 for i in range(256)]
    ks = [rnd.randrange(m) for _ in range(256)]
    ys, pf, g2 = world8.items(l, rows, ks)
    return l, rows, ks, ys, pf, g2


CORRUPTIONS = ["none", "one value", "one proof", "a commitment", "two adjacent rows", "two rows far apart", "every row"]


def _corrupt(kind, k, world8, rows, ks, ys, pf):
    """-> (commitments, ys, proofs, the bad items, the bad commitment rows)"""
    cm, ys, pf = list(world8.commitments[:8]), ys.copy(), list(pf)
    bad_items, bad_rows = set(), set()

    def bump(i):
        ys[i, 5] = k.fr.fr_from_int(k.fr.fr_to_int(ys[i, 5]) + 1)
        bad_items.add(i)

    if kind == "one value":
        bump(77)
    elif kind == "one proof":
        j = next(j for j in range(256) if (rows[j], ks[j]) != (rows[100], ks[100]))
        pf[100] = pf[j]
        bad_items.add(100)
    elif kind == "a commitment":
        cm[5] = world8.commitments[8]                                           # the constant polynomial's
        bad_rows.add(5)
        bad_items.update(i for i in range(256) if rows[i] == 5)
    elif kind == "two adjacent rows":
        bump(3), bump(4)                                                        # rows 3 and 4
    elif kind == "two rows far apart":
        bump(0), bump(255)                                                      # rows 0 and 7
    elif kind == "every row":
        for i in range(8):
            bump(16 + i)
    return cm, ys, pf, bad_items, bad_rows | {rows[i] for i in bad_items}


@pytest.mark.parametrize("kind", CORRUPTIONS)
def test_locate_names_exactly_the_planted_groups(k, world8, batch8, kind):
    """Grouped by commitment (8 groups), by item (256) and by an explicit array of 5 groups; weights derived.  The located set is the
    planted one, within 1 + 2 b ceil(log2 n_groups) pairing checks; the good batch costs exactly one."""
    l, rows, ks, ys, pf, g2 = batch8
    cm, ys, pf, bad_items, bad_rows = _corrupt(kind, k, world8, rows, ks, ys, pf)
    V = k.verifier
    five = [(i * 5) // 256 for i in range(256)]
    plans = (("commitment", None, 8, bad_rows), ("item", None, 256, bad_items), (five, 5, 5, {five[i] for i in bad_items}))
    assert V.verify_multiproof_batch(cm, rows, ks, ys, pf, world8.n, world8.srs, g2) is (not bad_items)
    for groups, n_groups, total, planted in plans:
        good, checks = V.locate_bad_multiproofs(cm, rows, ks, ys, pf, world8.n, world8.srs, g2, groups=groups, n_groups=n_groups)
        assert good.dtype == bool and good.shape == (total,)
        assert {int(g) for g in np.flatnonzero(~good)} == planted, (kind, total)
        assert 1 <= checks <= _bound(total, len(planted)), (kind, total, checks)
        if not planted:
            assert checks == 1


def test_locate_with_supplied_weights_and_empty_groups(k, world8, batch8):
    l, rows, ks, ys, pf, g2 = batch8
    cm, ys, pf, bad_items, _ = _corrupt("two rows far apart", k, world8, rows, ks, ys, pf)
    rp = k.verifier.compute_multiproof_r_powers(cm, rows, ks, ys, pf, world8.n)
    groups = [3 * r + 1 for r in rows]                                          # 26 groups of which 18 are empty, the first and the last among them
    good, checks = k.verifier.locate_bad_multiproofs(cm, rows, ks, ys, pf, world8.n, world8.srs, g2, r_powers=rp, groups=groups, n_groups=26)
    assert {int(g) for g in np.flatnonzero(~good)} == {1, 22} and checks <= _bound(26, 2)


# ---- 5. errors in the documented order, then a correct call on the same context --------------------------------------------------------
def test_error_table_in_the_documented_order_then_a_correct_call(k, world):
    L = k._lib
    lib = L.load()
    ctx = world.srs.ctx
    n, l = world.n, 16
    m = n // l
    rows, ks = [0, 1, 2, 1], [5, 6, 7, m - 1]
    ys, pf, g2 = world.items(l, rows, ks)
    cm = np.ascontiguousarray(np.stack(world.commitments[:3]))
    pf = np.ascontiguousarray(np.stack(pf))
    ci, ki, gi = np.array(rows, np.uint64), np.array(ks, np.uint64), np.array([0, 1, 1, 2], np.uint64)
    good = np.full(8, 7, np.uint8)
    bad, checks = L.sz(77), L.sz(77)
    small_srs = k.SRS.generate(TAU, 8)
    u8 = lambda a: None if a is None else a.ctypes.data_as(L.u8p)               # noqa: E731
    P_ = lambda a: None if a is None else L.ptr(a)                              # noqa: E731

    def call(ctx_h=ctx.handle, srs_h=world.srs.handle, cm_=cm, M=3, ci_=ci, ki_=ki, ys_=ys, pf_=pf, count=4, n_=n, l_=l, g2_=g2, gi_=gi, G=3, good_=good,
             bad_=C.byref(bad)):
        return lib.kzg_verify_multiproof_batch_locate(ctx_h, srs_h, P_(cm_), M, P_(ci_), P_(ki_), P_(ys_), P_(pf_), count, n_, l_, None, P_(g2_), P_(gi_), G,
                                                      u8(good_), bad_, C.byref(checks))

    lhs, rhs = np.full((3, 8), 7, np.uint64), np.full((3, 8), 7, np.uint64)
    linf, rinf = np.full(3, 7, np.uint8), np.full(3, 7, np.uint8)

    def sums(ctx_h=ctx.handle, srs_h=world.srs.handle, cm_=cm, M=3, ci_=ci, ki_=ki, ys_=ys, pf_=pf, count=4, n_=n, l_=l, gi_=gi, G=3, lhs_=lhs):
        return lib.kzg_coset_group_sums(ctx_h, srs_h, P_(cm_), M, P_(ci_), P_(ki_), P_(ys_), P_(pf_), count, n_, l_, None, P_(gi_), G, P_(lhs_), u8(linf), P_(rhs),
                                        u8(rinf))

    assert call() == L.OK and bad.value == 0 and checks.value == 1 and list(good[:3]) == [1, 1, 1]
    good[:] = 7
    bad.value = checks.value = 77
    for fn in (call, sums):
        for kw in (dict(ctx_h=None), dict(srs_h=None), dict(cm_=None), dict(ci_=None), dict(ki_=None), dict(ys_=None), dict(pf_=None), dict(gi_=None)):
            assert fn(**kw) == L.ERR_INVALID_ARG, kw                            # null pointers, group_indices among them
        assert fn(n_=96) == L.ERR_NOT_POWER_OF_TWO and fn(n_=1 << 25) == L.ERR_DOMAIN
        assert fn(l_=3) == L.ERR_INVALID_ARG
        assert fn(srs_h=small_srs.handle, gi_=np.array([0, 1, 1, 3], np.uint64)) == L.ERR_SRS_CAPACITY_EXCEEDED      # before the indices and groups
        assert fn(ki_=np.array([5, 6, 7, m], np.uint64)) == L.ERR_INVALID_ARG
        assert fn(gi_=np.array([0, 1, 1, 3], np.uint64)) == L.ERR_INVALID_ARG   # a group index = n_groups
        assert fn(G=0) == L.ERR_INVALID_ARG                                     # n_groups = 0 with count > 0
        huge = np.zeros((1 << 28) // l + 1, np.uint64)                          # never-touched zero pages: count * l > 2^28
        assert fn(ci_=huge, ki_=huge, gi_=huge, count=len(huge)) == L.ERR_TOO_LARGE
        assert fn(ci_=huge, ki_=huge, gi_=huge, count=len(huge), G=0) == L.ERR_INVALID_ARG                           # the group check comes first
        del huge
        off = pf.copy()
        off[2, 4] ^= 1
        assert fn(pf_=off) == L.ERR_G1_NOT_ON_CURVE
        offc = cm.copy()
        offc[1, 0] ^= 1
        assert fn(cm_=offc) == L.ERR_G1_NOT_ON_CURVE
    assert call(good_=None) == L.ERR_INVALID_ARG and call(bad_=None) == L.ERR_INVALID_ARG and sums(lhs_=None) == L.ERR_INVALID_ARG
    assert call(g2_=None) == L.ERR_INVALID_ARG                                  # consts::G2_TAU is [tau]_2 only
    bad_g2 = g2.copy()
    bad_g2[0] ^= 1
    off = pf.copy()
    off[2, 4] ^= 1
    assert call(pf_=off, g2_=bad_g2) == L.ERR_G1_NOT_ON_CURVE                   # a bad G1 point is reported before a bad G2 point
    assert call(g2_=bad_g2) == L.ERR_G2_TAU_NOT_ON_CURVE
    # n_groups > 2^28 with valid group indices: refused before anything of that size is allocated
    big_good = np.zeros(1, np.uint8)
    assert lib.kzg_verify_multiproof_batch_locate(ctx.handle, world.srs.handle, P_(cm), 3, P_(ci), P_(ki), P_(ys), P_(pf), 4, n, l, None, P_(g2), P_(gi),
                                                  (1 << 28) + 1, u8(big_good), C.byref(bad), C.byref(checks)) == L.ERR_TOO_LARGE
    assert (good == 7).all() and bad.value == 77 and checks.value == 77 and (lhs == 7).all() and (linf == 7).all()  # no error path writes an output
    # count = 0: every group good, nothing bad, no pairing check -- even with a g2 point off the twist nothing is looked at
    assert call(count=0, cm_=None, ci_=None, ki_=None, ys_=None, pf_=None, gi_=None, G=8, g2_=bad_g2) == L.OK
    assert (good == 1).all() and bad.value == 0 and checks.value == 0
    assert sums(count=0, cm_=None, ci_=None, ki_=None, ys_=None, pf_=None, gi_=None) == L.OK
    assert not lhs.any() and not rhs.any() and (linf == 1).all() and (rinf == 1).all()
    good_v, n_checks = k.verifier.locate_bad_multiproofs(world.commitments[:3], [], [], np.zeros((0, l, 4), np.uint64), [], n, world.srs, g2, groups="commitment")
    assert good_v.all() and good_v.shape == (3,) and n_checks == 0
    # the Python surface maps the errors as the batch entry's does
    with pytest.raises(k.errors.NotOnCurveError, match="G1 point not on curve"):
        k.verifier.locate_bad_multiproofs(world.commitments[:3], rows, ks, ys, list(off), n, world.srs, g2)
    with pytest.raises(ValueError):
        k.verifier.coset_group_sums(world.commitments[:3], rows, ks, ys, list(pf), n, world.srs, groups=[0, 1, 2, 3], n_groups=3)
    # ... and the context still works
    assert call() == L.OK and bad.value == 0 and checks.value == 1
    worse = ys.copy()
    worse[2, 0] = k.fr.fr_from_int(1)
    assert call(ys_=worse) == L.OK and bad.value == 1 and list(good[:3]) == [1, 0, 1] and checks.value <= _bound(3, 1)
    small_srs.close()


# ---- 6. the bound-checked build: cases 1 and 4 at l = 16 with every site counter at 0 -------------------------------------------------
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
rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", "-x", "-k", %(select)r, *%(tests)r])
counts = (C.c_ulonglong * n)()
first = (C.c_int32 * (9 * n))()
assert h.kzg_bc_read_all(counts, first) == 0
print("PYTEST_RC", int(rc))
for s in range(n):
    print("SITE", s, counts[s])
'''
WORKLOAD = ["tests/test_gpu_multiproof_locate.py::" + t for t in ("test_group_sums_are_bit_equal_to_big_integers", "test_locate_names_exactly_the_planted_groups")]
SELECT = "16- or test_locate_names"                                            # the l = 16 cases of test 1 (ids "16-<count>"), all of test 4


def test_bound_checked_build_keeps_every_precondition():
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": WORKLOAD, "select": SELECT}], capture_output=True, text=True, timeout=1500,
                         env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "PYTEST_RC 0" in out, (out[-3000:], res.stderr[-2000:])
    assert " passed" in out and "no tests ran" not in out, out[-2000:]
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert sites
    fired = {int(s[1]): int(s[2]) for s in sites if int(s[2])}
    assert not fired, fired
