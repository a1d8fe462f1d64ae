"""-m gpu: coset proofs of MIXED blob shapes in one call (`kzg_coset_interpolate_rlc_mixed`, `kzg_verify_multiproof_batch_mixed`): the
ragged interpolation kernel bit-equal to big integers and to the field sum of one uniform call per class, the same bits under another item
order and class numbering, verdicts on a known-tau SRS (accept, every single fault rejects, derived and supplied weights agree), one class
against `kzg_verify_multiproof_batch`, the error table in its documented order, degenerate inputs, threads, and the bound-checked build."""
import ctypes as C
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

import coset_mixed_ref
import pyref
from pyref import R_

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TAU = int.from_bytes(__import__("hashlib").sha256(b"kzg-bn254-mi355x/multiproof-verify/v1").digest(), "big") % R_


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


# ---- 1, 2. the ragged interpolation against big integers ---------------------------------------------------------------------------------
# class (n, l), items: the smallest counts that cross each edge of the kernel (under 8 000 values in all)
EDGE_CLASSES = [
    ((2, 1), 2),                 # smallest domain
    ((1 << 5, 1), 513),          # one item past a 512-coset tile
    ((1 << 5, 16), 33),          # l = n / 2, one past a 32-coset tile
    ((1 << 12, 16), 31),
    ((1 << 14, 16), 3),          # same l, other n, coset indices >= 2^12 / 16: a shared-m bug shows
    ((1 << 12, 64), 9),
    ((1 << 11, 512), 2),         # one coset per tile
    ((1 << 12, 1024), 2),        # second launch
    ((1 << 13, 2048), 1),        # per-coset route
    ((1 << 24, 16), 2),          # k = m - 1 and m - 2, largest domain, table shift
    ((1 << 8, 4), 0),            # empty class
]


class Edge:
    """The items of EDGE_CLASSES shuffled with a fixed seed, and A_t by big integers -- computed once, never changed."""

    def __init__(self):
        rnd = random.Random(20240)
        self.classes = [c for c, _ in EDGE_CLASSES]
        special = [0, 1, R_ - 1]
        items = []
        for s, ((n, l), count) in enumerate(EDGE_CLASSES):
            m = n // l
            for j in range(count):
                k_ = rnd.randrange(m)
                if n == 1 << 14:
                    k_ = (1 << 12) // 16 + rnd.randrange(m - (1 << 12) // 16)
                if n == 1 << 24:
                    k_ = m - 1 - j
                ys = [rnd.choice(special) if rnd.random() < 0.05 else rnd.randrange(R_) for _ in range(l)]
                w = rnd.choice(special) if rnd.random() < 0.05 else rnd.randrange(R_)
                items.append((s, k_, ys, w))
        rnd.shuffle(items)
        self.items = items
        assert sum(len(it[2]) for it in items) < 8000
        self.want = coset_mixed_ref.mixed_rlc(self.classes, [it[0] for it in items], [it[1] for it in items], [it[2] for it in items],
                                              [it[3] for it in items])

    def run(self, k, items=None, classes=None):
        items = self.items if items is None else items
        classes = self.classes if classes is None else classes
        return k.helpers.coset_interpolate_rlc_mixed(classes, [it[0] for it in items], [it[1] for it in items],
                                                     [pyref.frs_to_mont(it[2]) for it in items], pyref.frs_to_mont([it[3] for it in items]))


@pytest.fixture(scope="module")
def edge():
    return Edge()


def test_mixed_interpolation_is_bit_equal_to_big_integers_and_to_the_sum_of_uniform_calls(k, edge):
    got = edge.run(k)
    assert got.shape == (2048, 4) and got.dtype == np.uint64
    assert np.array_equal(got, pyref.frs_to_mont(edge.want))
    acc = [0] * 2048
    for s, (n, l) in enumerate(edge.classes):
        mine = [it for it in edge.items if it[0] == s]
        if not mine:
            continue
        part = k.helpers.coset_interpolate_rlc(np.stack([pyref.frs_to_mont(it[2]) for it in mine]), [it[1] for it in mine],
                                               pyref.frs_to_mont([it[3] for it in mine]), n)
        for t, v in enumerate(pyref.frs_from_mont(part)):
            acc[t] = (acc[t] + v) % R_
    assert acc == edge.want
    # an empty LONGEST class still sets l_max: its columns are zero; no item at all: zeros
    longer = edge.classes + [(1 << 13, 4096)]
    again = edge.run(k, classes=longer)
    assert again.shape == (4096, 4) and np.array_equal(again[:2048], got) and not again[2048:].any()
    assert not k.helpers.coset_interpolate_rlc_mixed(edge.classes, [], [], [], np.zeros((0, 4), np.uint64)).any()


def test_same_bits_after_reshuffling_the_items_and_renumbering_the_classes(k, edge):
    got = edge.run(k)
    rnd = random.Random(77)
    order = list(range(len(edge.classes)))
    rnd.shuffle(order)                                                 # new class number q holds the old class order[q]
    new_of_old = {old: q for q, old in enumerate(order)}
    items = [(new_of_old[s], k_, ys, w) for s, k_, ys, w in edge.items]
    rnd.shuffle(items)
    assert np.array_equal(edge.run(k, items, [edge.classes[o] for o in order]), got)
    # a class split in two numbers (repeated class rows)
    dup = edge.classes + [edge.classes[1]]
    items = [((len(dup) - 1) if (s == 1 and i % 2) else s, k_, ys, w) for i, (s, k_, ys, w) in enumerate(edge.items)]
    assert np.array_equal(edge.run(k, items, dup), got)


# ---- 3. verdicts on a known-tau SRS -------------------------------------------------------------------------------------------------------
BLOB_SHAPES = [(1 << 6, 1), (1 << 8, 16), (1 << 8, 16), (1 << 10, 16), (1 << 12, 256)]      # one blob each: two at (2^8, 16)
V_CLASSES = [(1 << 6, 1), (1 << 8, 16), (1 << 10, 16), (1 << 12, 256)]
BLOB_CLASS = [0, 1, 1, 2, 3]


class World:
    def __init__(self, k, ctx=None):
        self.k = k
        self.srs = k.SRS.generate(TAU, 4096, ctx) if ctx is not None else k.SRS.generate(TAU, 4096)
        self.commitments, self.cosets, self.proofs = [], [], []
        for b, (n, l) in enumerate(BLOB_SHAPES):
            kz = k.KZG.new(ctx) if ctx is not None else k.KZG.new()
            kz.calculate_and_store_roots_of_unity(n * 32)
            rnd = random.Random(3000 + b)
            poly = k.PolynomialEvalForm(pyref.frs_to_mont([rnd.randrange(R_) for _ in range(n)]))
            self.commitments.append(kz.commit_eval_form(poly, self.srs))
            self.cosets.append(kz.cosets(poly, l))
            self.proofs.append(kz.compute_multiproofs(poly, self.srs, l))
        self.g2 = [self.g2_at(l) for _, l in V_CLASSES]
        self.all = [(b, kk) for b, (n, l) in enumerate(BLOB_SHAPES) for kk in range(n // l)]     # 64 + 16 + 16 + 64 + 16 items

    def g2_at(self, l):
        return self.k.helpers.g2_mul_generator(self.k.fr.fr_from_int(pow(TAU, l, R_)))

    def args(self, picks):
        """picks: (blob, coset) pairs -> rows, class indices, coset indices, ragged values, proofs"""
        return ([b for b, _ in picks], [BLOB_CLASS[b] for b, _ in picks], [kk for _, kk in picks], [self.cosets[b][kk] for b, kk in picks],
                [self.proofs[b][kk] for b, kk in picks])

    def verify(self, rows, si, ks, ys, pf, g2=None, r_powers=None, classes=V_CLASSES, commitments=None, ctx=None):
        return self.k.verifier.verify_multiproof_batch_mixed(self.commitments if commitments is None else commitments, rows, classes, si, ks, ys, pf,
                                                             self.srs, self.g2 if g2 is None else g2, r_powers, ctx)

    def both(self, rows, si, ks, ys, pf, g2=None):
        """derived and supplied weights agree"""
        a = self.verify(rows, si, ks, ys, pf, g2)
        rp = self.k.verifier.compute_multiproof_r_powers_mixed(self.commitments, rows, V_CLASSES, si, ks, ys, pf)
        b = self.verify(rows, si, ks, ys, pf, g2, r_powers=rp)
        assert a is b
        return a


@pytest.fixture(scope="module")
def world(k):
    return World(k)


def test_all_items_and_a_shuffled_subset_are_accepted(k, world):
    assert world.both(*world.args(world.all)) is True
    rnd = random.Random(31)
    picks = rnd.sample(world.all, 60) + [(0, 0), (1, 6), (3, 1), (4, 2)]
    picks[5] = picks[1]                                                # a repeated item
    rnd.shuffle(picks)
    assert len({BLOB_CLASS[b] for b, _ in picks}) == 4
    assert world.both(*world.args(picks)) is True
    # the flat form of the values is the same call
    rows, si, ks, ys, pf = world.args(picks)
    assert world.verify(rows, si, ks, np.concatenate(ys), pf) is True
    # one class only, and classes numbered otherwise (with an empty class in front)
    only = [p for p in picks if BLOB_CLASS[p[0]] == 2]
    assert world.both(*world.args(only)) is True
    classes = [(1 << 9, 32)] + V_CLASSES[::-1]
    g2 = [world.g2_at(32)] + world.g2[::-1]
    assert world.verify(rows, [4 - s for s in si], ks, ys, pf, g2=g2, classes=classes) is True


def test_one_fault_at_a_time_rejects(k, world):
    rnd = random.Random(32)
    picks = rnd.sample(world.all, 48) + [(0, 63), (1, 15), (2, 0), (3, 40), (4, 7)]
    rnd.shuffle(picks)
    rows, si, ks, ys, pf = world.args(picks)
    assert world.both(rows, si, ks, ys, pf) is True
    for s in range(4):
        i = si.index(s)
        n, l = V_CLASSES[s]
        bad = [y.copy() for y in ys]
        bad[i][l - 1] = k.fr.fr_from_int(k.fr.fr_to_int(bad[i][l - 1]) + 1)
        assert world.both(rows, si, ks, bad, pf) is False, ("value", s)
        j = next(j for j in range(len(picks)) if picks[j] != picks[i])
        badp = list(pf)
        badp[i] = pf[j]
        assert world.both(rows, si, ks, ys, badp) is False, ("proof", s)
        badk = list(ks)
        badk[i] = (badk[i] + 1) % (n // l)
        assert world.both(rows, si, badk, ys, pf) is False, ("coset index", s)
    # an item's class moved between the two l = 16 classes: (2^8, 16) -> (2^10, 16), its coset index valid in both
    i = next(i for i, s in enumerate(si) if s == 1 and ks[i] != 0)
    moved = list(si)
    moved[i] = 2
    assert world.both(rows, moved, ks, ys, pf) is False
    # its commitment row: the other blob of the same shape
    rows2 = list(rows)
    rows2[i] = 3 - rows2[i]
    assert world.both(rows2, si, ks, ys, pf) is False
    # one class's G2 point replaced by [tau^(2 l)]_2 (class 1 and class 2 share l = 16: both entries, or step 8 refuses the call)
    for s in (0, 3):
        g2 = list(world.g2)
        g2[s] = world.g2_at(2 * V_CLASSES[s][1])
        assert world.both(rows, si, ks, ys, pf, g2) is False, ("g2", s)
    g2 = list(world.g2)
    g2[1] = g2[2] = world.g2_at(32)
    assert world.both(rows, si, ks, ys, pf, g2) is False
    assert world.both(rows, si, ks, ys, pf) is True


# ---- 4. one class, supplied weights: the verdict of the uniform entry -----------------------------------------------------------------------
def test_one_class_with_supplied_weights_agrees_with_the_uniform_entry(k, world):
    V = k.verifier
    for b in (0, 3, 4):
        n, l = BLOB_SHAPES[b]
        picks = [(b, kk) for kk in random.Random(b).sample(range(n // l), 12)]
        rows, si, ks, ys, pf = world.args(picks)
        s = BLOB_CLASS[b]
        g2 = world.g2[s]
        rp = V.compute_multiproof_r_powers(world.commitments, rows, ks, np.stack(ys), pf, n)
        bad = [y.copy() for y in ys]
        bad[4][0] = k.fr.fr_from_int(k.fr.fr_to_int(bad[4][0]) + 1)
        for values, want in ((ys, True), (bad, False)):
            uniform = V.verify_multiproof_batch(world.commitments, rows, ks, np.stack(values), pf, n, world.srs, g2, rp)
            mixed = V.verify_multiproof_batch_mixed(world.commitments, rows, [(n, l)], [0] * 12, ks, values, pf, world.srs, [g2], rp)
            assert uniform is want and mixed is want, (b, want)


# ---- 5. the error table, degenerate inputs, threads ------------------------------------------------------------------------------------------
def test_error_table_in_the_documented_order(k, world, test_srs_wire):
    L = k._lib
    lib = L.load()
    ctx = world.srs.ctx
    picks = [(0, 5), (1, 6), (3, 7), (4, 15), (2, 3)]
    rows, si, ks, ys, pf = world.args(picks)
    cm = np.ascontiguousarray(np.stack(world.commitments))
    pfa = np.ascontiguousarray(np.stack(pf))
    ysa = np.ascontiguousarray(np.concatenate(ys))
    cn = np.array([c[0] for c in V_CLASSES], np.uint64)
    cl = np.array([c[1] for c in V_CLASSES], np.uint64)
    ci, sia, ki = np.array(rows, np.uint64), np.array(si, np.uint64), np.array(ks, np.uint64)
    g2 = np.ascontiguousarray(np.stack(world.g2))
    ok = L.i32(7)
    lag = world.srs.lagrange(64)
    other_ctx = L.Context(0)
    other_srs = k.SRS(test_srs_wire[:64], order=64, ctx=other_ctx)
    small_srs = k.SRS(test_srs_wire[:64], order=64)                            # l_max = 256 > 64 points
    keep = []

    def call(ctx_h=ctx.handle, srs_h=world.srs.handle, cm_=cm, M=5, ci_=ci, cn_=cn, cl_=cl, S=4, si_=sia, ki_=ki, ys_=ysa, pf_=pfa, count=5, g2_=g2,
             ok_=C.byref(ok)):
        keep.extend([cm_, ci_, cn_, cl_, si_, ki_, ys_, pf_, g2_])
        P = lambda a: None if a is None else L.ptr(a)                          # noqa: E731
        return lib.kzg_verify_multiproof_batch_mixed(ctx_h, srs_h, P(cm_), M, P(ci_), P(cn_), P(cl_), S, P(si_), P(ki_), P(ys_), P(pf_), count, None, P(g2_), ok_)

    u64 = lambda *v: np.array(v, np.uint64)                                    # noqa: E731
    assert call() == L.OK and ok.value == 1
    ok.value = 7
    bad_n = u64(64, 96, 1 << 10, 1 << 12)
    # 1. null pointers, foreign or Lagrange SRS -- in front of everything else
    for kw in (dict(ctx_h=None), dict(srs_h=None), dict(ok_=None), dict(cm_=None), dict(ci_=None), dict(cn_=None), dict(cl_=None), dict(si_=None),
               dict(ki_=None), dict(ys_=None), dict(pf_=None), dict(g2_=None), dict(srs_h=other_srs.handle), dict(srs_h=lag.handle)):
        assert call(**dict(dict(cn_=bad_n), **kw)) == L.ERR_INVALID_ARG, kw
    # 2. no class, items;  3. more than 512 classes, in front of a broken class
    assert call(S=0) == L.ERR_INVALID_ARG
    many_n, many_l, many_g2 = np.full(513, 64, np.uint64), np.full(513, 16, np.uint64), np.zeros((513, 16), np.uint64)
    many_n[1] = 96
    assert call(cn_=many_n, cl_=many_l, S=513, g2_=many_g2) == L.ERR_TOO_LARGE
    assert call(cn_=many_n, cl_=many_l, S=512, g2_=many_g2) == L.ERR_NOT_POWER_OF_TWO
    # 4. every class in class order with coset_domain_check's codes, in front of the SRS capacity
    assert call(cn_=bad_n, srs_h=small_srs.handle) == L.ERR_NOT_POWER_OF_TWO
    assert call(cn_=u64(64, 1 << 25, 96, 1 << 12), cl_=u64(1, 3, 16, 256)) == L.ERR_DOMAIN      # class 1 before class 2, the domain before the chunk
    for cl_bad in (u64(1, 3, 16, 256), u64(1, 0, 16, 256), u64(1, 256, 16, 256), u64(64, 16, 16, 256)):
        assert call(cl_=cl_bad, srs_h=small_srs.handle) == L.ERR_INVALID_ARG, cl_bad
    assert call(cn_=u64(64, 1, 1 << 10, 1 << 12)) == L.ERR_INVALID_ARG
    # 5. l_max over ALL classes against the SRS, in front of the indices
    assert call(srs_h=small_srs.handle, ki_=u64(64, 6, 7, 15, 3)) == L.ERR_SRS_CAPACITY_EXCEEDED
    assert call(cn_=u64(64, 256, 1 << 10, 1 << 14), cl_=u64(1, 16, 16, 8192), si_=u64(0, 1, 1, 1, 2), ki_=u64(5, 6, 7, 15, 3)) == L.ERR_SRS_CAPACITY_EXCEEDED   # an EMPTY class
    # 6. class, coset and commitment indices, in front of the total
    assert call(si_=u64(0, 1, 4, 3, 2)) == L.ERR_INVALID_ARG
    assert call(ki_=u64(64, 6, 7, 15, 3)) == L.ERR_INVALID_ARG
    assert call(ki_=u64(5, 16, 7, 15, 3)) == L.ERR_INVALID_ARG                  # 16 = m of class 1, valid in class 2
    assert call(ci_=u64(0, 1, 5, 4, 2)) == L.ERR_INVALID_ARG
    assert call(M=4) == L.ERR_INVALID_ARG
    # 7. the total of the chunk lengths (never-touched zero pages), in front of 8. the G2 points of classes 1 and 2 (l = 16 both) differing
    differ = g2.copy()
    differ[2] = g2[0]
    huge = np.zeros((1 << 28) // 256 + 1, np.uint64)
    huge_s = np.full(len(huge), 3, np.uint64)
    assert call(ci_=huge, si_=huge_s, ki_=huge, count=len(huge), g2_=differ) == L.ERR_TOO_LARGE
    del huge, huge_s
    keep.clear()
    off = pfa.copy()
    off[2, 4] ^= 1
    assert call(g2_=differ) == L.ERR_INVALID_ARG
    assert call(g2_=differ, pf_=off) == L.ERR_INVALID_ARG                       # 8 in front of 9
    # 9. G1 off the curve, in front of 10. G2 off the twist (classes with items only, in class order)
    bad_g2 = g2.copy()
    bad_g2[0, 0] ^= 1
    assert call(pf_=off) == L.ERR_G1_NOT_ON_CURVE
    assert call(pf_=off, g2_=bad_g2) == L.ERR_G1_NOT_ON_CURVE
    offc = cm.copy()
    offc[1, 0] ^= 1
    assert call(cm_=offc) == L.ERR_G1_NOT_ON_CURVE
    assert call(g2_=bad_g2) == L.ERR_G2_TAU_NOT_ON_CURVE
    with_empty = np.concatenate([g2, bad_g2[:1]])                               # a fifth, EMPTY class whose point is off the twist: not tested
    assert call(cn_=u64(64, 256, 1 << 10, 1 << 12, 128), cl_=u64(1, 16, 16, 256, 8), S=5, g2_=with_empty) == L.OK and ok.value == 1
    ok.value = 7
    assert call(g2_=bad_g2) == L.ERR_G2_TAU_NOT_ON_CURVE
    assert ok.value == 7                                                       # no error path writes the verdict
    # count = 0: accepted with no device work (whatever the item pointers), the class table still checked
    assert call(count=0, cm_=None, ci_=None, si_=None, ki_=None, ys_=None, pf_=None) == L.OK and ok.value == 1
    ok.value = 7
    assert call(count=0, cn_=bad_n) == L.ERR_NOT_POWER_OF_TWO
    # kzg_coset_interpolate_rlc_mixed's own table
    one = pyref.frs_to_mont([1] * 5)
    out = np.zeros((256, 4), np.uint64)

    def rlc(ctx_h=ctx.handle, cn_=cn, cl_=cl, S=4, si_=sia, ki_=ki, ys_=ysa, w_=one, out_=out):
        P = lambda a: None if a is None else L.ptr(a)                          # noqa: E731
        return lib.kzg_coset_interpolate_rlc_mixed(ctx_h, P(cn_), P(cl_), S, P(si_), P(ki_), P(ys_), P(w_), 5, P(out_))

    assert rlc() == L.OK
    for kw in (dict(ctx_h=None), dict(cn_=None), dict(cl_=None), dict(si_=None), dict(ki_=None), dict(ys_=None), dict(w_=None), dict(out_=None), dict(S=0),
               dict(cl_=u64(1, 3, 16, 256)), dict(si_=u64(0, 1, 4, 3, 2)), dict(ki_=u64(64, 6, 7, 15, 3))):
        assert rlc(**kw) == L.ERR_INVALID_ARG, kw
    assert rlc(cn_=bad_n) == L.ERR_NOT_POWER_OF_TWO and rlc(cn_=u64(64, 1 << 25, 1 << 10, 1 << 12)) == L.ERR_DOMAIN
    # the Python surface maps them as _raise_for does; every error left the context usable
    with pytest.raises(k.errors.NotOnCurveError, match="G1 point not on curve"):
        world.verify(rows, si, ks, ys, list(off))
    with pytest.raises(k.errors.NotOnCurveError, match="G2_TAU not on curve"):
        world.verify(rows, si, ks, ys, pf, g2=list(bad_g2))
    with pytest.raises(ValueError):
        world.verify(rows, si, [64] + ks[1:], ys, pf)
    assert call() == L.OK and ok.value == 1
    lag.close(); other_srs.close(); small_srs.close(); other_ctx.close()


def test_identity_commitment_and_identity_proofs(k, world):
    """A constant polynomial has identity proofs, the zero polynomial the identity commitment too; both in two classes of one call."""
    commitments, rows, si, ks, ys, pf = [], [], [], [], [], []
    for c, (value, (n, l)) in enumerate(((12345, V_CLASSES[1]), (0, V_CLASSES[2]), (777, V_CLASSES[0]))):
        kz = k.KZG.new()
        kz.calculate_and_store_roots_of_unity(n * 32)
        poly = k.PolynomialEvalForm(pyref.frs_to_mont([value] * n))
        cmt = kz.commit_eval_form(poly, world.srs)
        proofs = kz.compute_multiproofs(poly, world.srs, l)
        assert not proofs.any() and k.fr.g1_is_identity(cmt) == (value == 0)
        commitments.append(cmt)
        co = kz.cosets(poly, l)
        for kk in (0, 1, n // l - 1):
            rows.append(c); si.append(V_CLASSES.index((n, l))); ks.append(kk); ys.append(co[kk]); pf.append(proofs[kk])
    assert world.verify(rows, si, ks, ys, pf, commitments=commitments) is True
    swapped = [(r + 1) % 3 for r in rows]
    assert world.verify(swapped, si, ks, ys, pf, commitments=commitments) is False
    assert world.verify([], [], [], [], [], commitments=commitments) is True
    assert world.verify([], [], [], [], [], commitments=[]) is True


def test_two_threads_on_one_context(k, world):
    """Verdicts of a valid and a faulted mixed batch are unchanged when two threads share the context (the weights are derived on the host
    pool in front of the context's lock), a uniform call between them."""
    rnd = random.Random(41)
    picks = rnd.sample(world.all, 40)
    rows, si, ks, ys, pf = world.args(picks)
    bad = [y.copy() for y in ys]
    bad[9][0] = k.fr.fr_from_int(1)
    b, kk = world.all[100]
    n, l = BLOB_SHAPES[b]
    errors, results = [], {}

    def run(name):
        try:
            out = []
            for _ in range(4):
                out.append((world.verify(rows, si, ks, ys, pf), world.verify(rows, si, ks, bad, pf),
                            k.verifier.verify_multiproof(world.commitments[b], world.proofs[b][kk], kk, world.cosets[b][kk], n, world.srs,
                                                         world.g2[BLOB_CLASS[b]])))
            results[name] = out
        except Exception as e:                                                  # reported below
            errors.append((name, repr(e)))

    ts = [threading.Thread(target=run, args=(nm,)) for nm in ("a", "b")]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert results["a"] == [(True, False, True)] * 4 and results["b"] == [(True, False, True)] * 4


# ---- 6. the bound-checked build runs cases 1 and 3 with every site counter at 0 ------------------------------------------------------------
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
WORKLOAD = ["tests/test_gpu_multiproof_verify_mixed.py::" + t for t in (
    "test_mixed_interpolation_is_bit_equal_to_big_integers_and_to_the_sum_of_uniform_calls",
    "test_same_bits_after_reshuffling_the_items_and_renumbering_the_classes",
    "test_all_items_and_a_shuffled_subset_are_accepted", "test_one_fault_at_a_time_rejects")]


def test_bound_checked_build_keeps_every_precondition():
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": WORKLOAD}], capture_output=True, text=True, timeout=900,
                         env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "PYTEST_RC 0" in out, (out[-3000:], res.stderr[-2000:])
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert sites
    fired = {int(s[1]): int(s[2]) for s in sites if int(s[2])}
    assert not fired, fired
