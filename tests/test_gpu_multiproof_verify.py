"""-m gpu: verification of the FK20 coset proofs (`kzg_coset_interpolate_rlc`, `kzg_verify_multiproof`, `kzg_verify_multiproof_batch`):
the interpolation kernel bit-equal to big integers, round trips with `compute_multiproofs` on a known-tau SRS, rejection of every single
fault, degenerate inputs and the error table, the mainnet `g2_tau_l = None` path, threads and contexts at once, and the bound-checked
build.  Everything that must ACCEPT uses an SRS generated from a known tau (`SRS.generate`) with g2_tau_l = [tau^l]G2 from
`g2_mul_generator`; the reference's 3 000-point test SRS (whose tau is not the mainnet one) appears only where both paths must reject."""
import ctypes as C
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

import coset_ref
import pyref
from pyref import R_

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TAU = int.from_bytes(__import__("hashlib").sha256(b"kzg-bn254-mi355x/multiproof-verify/v1").digest(), "big") % R_
N_DOMAIN = 4096


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


def rand_ints(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R_) for _ in range(n)]


def kzg_for(k, n, ctx=None):
    kzg = k.KZG.new(ctx) if ctx is not None else k.KZG.new()
    kzg.calculate_and_store_roots_of_unity(n * 32)
    return kzg


class World:
    """Three random polynomials of 4 096 evaluations on a known-tau SRS; per chunk length their proofs and cosets."""

    def __init__(self, k, ctx=None):
        self.k, self.n = k, N_DOMAIN
        self.srs = k.SRS.generate(TAU, self.n, ctx) if ctx is not None else k.SRS.generate(TAU, self.n)
        self.kz = kzg_for(k, self.n, ctx)
        self.polys = [k.PolynomialEvalForm(pyref.frs_to_mont(rand_ints(self.n, 900 + i))) for i in range(3)]
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

    def verify(self, l, rows, ks, ys, pf, g2, r_powers=None, commitments=None, ctx=None):
        return self.k.verifier.verify_multiproof_batch(self.commitments if commitments is None else commitments, rows, ks, ys, pf, self.n,
                                                       self.srs, g2, r_powers, ctx)


@pytest.fixture(scope="module")
def world(k):
    return World(k)


# ---- 5. the interpolation kernel against big integers ---------------------------------------------------------------------------
def _rlc_case(k, log_n, l, count, seed, equal_k=False):
    n, m = 1 << log_n, (1 << log_n) // l
    rnd = random.Random(seed)
    special = [0, 1, R_ - 1]
    ys = [[rnd.choice(special) if rnd.random() < 0.05 else rnd.randrange(R_) for _ in range(l)] for _ in range(count)]
    ws = [rnd.choice(special) if rnd.random() < 0.1 else rnd.randrange(R_) for _ in range(count)]
    ks = [rnd.randrange(m) for _ in range(count)]
    ys[0][0], ws[0] = R_ - 1, R_ - 1
    ks[0] = m - 1
    if count > 2:
        ys[1], ws[2], ks[1] = [0] * l, 0, 0
    if equal_k:
        ks = [ks[0]] * count
    got = k.helpers.coset_interpolate_rlc(np.stack([pyref.frs_to_mont(v) for v in ys]), ks, pyref.frs_to_mont(ws), n)
    want = pyref.frs_to_mont(coset_ref.coset_rlc(ys, ks, ws, n))
    assert got.shape == (l, 4) and got.dtype == np.uint64
    assert np.array_equal(got, want), (log_n, l, count)
    return ys, ws, ks, got


@pytest.mark.parametrize("l,count", [(l, c) for l in (1, 2, 16, 64, 1024, 2048) for c in (1, 3, 257, 4096) if c < 4096 or l <= 64])
def test_coset_interpolate_rlc_is_bit_equal_to_big_integers(k, l, count):
    """No SRS involved.  n = 2^12; l = 2048 takes the per-coset NTT fallback; 4 096 items at l <= 64."""
    _rlc_case(k, 12, l, count, 5000 + 13 * l + count)


def test_coset_interpolate_rlc_equal_indices_and_item_order(k):
    """All-equal coset indices; the same items in two orders (another split into tiles and workgroups) give the same bits."""
    for l, count in ((1, 1500), (16, 700), (64, 300), (1024, 5)):
        ys, ws, ks, got = _rlc_case(k, 12, l, count, 6000 + l, equal_k=(l != 16))
        perm = list(range(count))
        random.Random(l).shuffle(perm)
        again = k.helpers.coset_interpolate_rlc(np.stack([pyref.frs_to_mont(ys[i]) for i in perm]), [ks[i] for i in perm],
                                                pyref.frs_to_mont([ws[i] for i in perm]), 4096)
        assert np.array_equal(again, got)
    assert not k.helpers.coset_interpolate_rlc(np.zeros((0, 16, 4), np.uint64), [], np.zeros((0, 4), np.uint64), 4096).any()


def test_coset_interpolate_rlc_at_the_largest_domain_without_an_n_sized_table(k):
    """n = 2^24, l = 16, coset indices up to m - 1 = 2^20 - 1.  The twist comes from the factored tables (2^10 + 2^14 entries, 0.6 MiB),
    so device memory must not grow with n: a table of w^-e for every e < n would be 512 MiB; 64 MiB is allowed for everything."""
    import torch
    log_n, l = 24, 16
    m = (1 << log_n) // l
    _rlc_case(k, log_n, l, 3, 7001)                                             # builds the tables (and the buffers of this size)
    free_before = torch.cuda.mem_get_info()[0]
    rnd = random.Random(7002)
    count = 300
    ys = [[rnd.randrange(R_) for _ in range(l)] for _ in range(count)]
    ws = [rnd.randrange(R_) for _ in range(count)]
    ks = [m - 1, m - 2, 1, 0] + [rnd.randrange(m) for _ in range(count - 4)]
    got = k.helpers.coset_interpolate_rlc(np.stack([pyref.frs_to_mont(v) for v in ys]), ks, pyref.frs_to_mont(ws), 1 << log_n)
    assert np.array_equal(got, pyref.frs_to_mont(coset_ref.coset_rlc(ys, ks, ws, 1 << log_n)))
    assert free_before - torch.cuda.mem_get_info()[0] < (64 << 20)


# ---- 6. round trips with compute_multiproofs on the known-tau SRS ---------------------------------------------------------------
@pytest.mark.parametrize("l", [1, 16, 256, 2048])
def test_every_proof_of_compute_multiproofs_verifies(k, world, l):
    """Known-tau SRS.  Singly (32 sampled cosets), all m cosets of one polynomial in one batch, and the three polynomials shuffled with
    repeats in one batch.  At l = 1 `verify_multiproof` agrees with `verify_proof(C, pi, y, w^k)` on accepting and rejecting inputs."""
    n, m = world.n, world.n // l
    proofs, cosets, g2 = world.at(l)
    V = k.verifier
    rnd = random.Random(l)
    sample = sorted(set([0, m - 1] + [rnd.randrange(m) for _ in range(30)]))[:32]
    for i, kk in enumerate(sample):
        c = i % 3
        assert V.verify_multiproof(world.commitments[c], proofs[c][kk], kk, cosets[c][kk], n, world.srs, g2) is True
    assert V.verify_multiproof(world.commitments[1], proofs[0][sample[0]], sample[0], cosets[0][sample[0]], n, world.srs, g2) is False
    if l == 1:
        roots = world.kz.get_roots_of_unities()
        g2_tau = g2
        for kk in sample[:6]:
            y, z, pi = cosets[0][kk][0], roots[kk], proofs[0][kk]
            assert V.verify_proof(world.commitments[0], pi, y, z, g2_tau) is True
            assert V.verify_multiproof(world.commitments[0], pi, kk, [y], n, world.srs, g2) is True
            other = roots[(kk + 1) % n]
            assert V.verify_proof(world.commitments[0], pi, y, other, g2_tau) is False
            assert V.verify_multiproof(world.commitments[0], pi, (kk + 1) % n, [y], n, world.srs, g2) is False
            y_bad = k.fr.fr_from_int(k.fr.fr_to_int(y) + 1)
            assert V.verify_proof(world.commitments[0], pi, y_bad, z, g2_tau) is False
            assert V.verify_multiproof(world.commitments[0], pi, kk, [y_bad], n, world.srs, g2) is False
    ks = list(range(m))
    ys, pf, _ = world.items(l, [2] * m, ks)
    assert world.verify(l, [2] * m, ks, ys, pf, g2) is True
    rows = [rnd.randrange(3) for _ in range(200)]
    ks = [rnd.randrange(m) for _ in range(200)]
    rows[50:60], ks[50:60] = rows[0:10], ks[0:10]                               # repeats
    ys, pf, _ = world.items(l, rows, ks)
    assert world.verify(l, rows, ks, ys, pf, g2) is True


# ---- 7. one fault in an otherwise valid batch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", [1, 16, 256])
def test_a_single_fault_rejects_the_batch(k, world, l):
    """Known-tau SRS; batches of 96 valid items with exactly one fault each: KZG_OK with out_ok = 0, with derived and with supplied
    r_powers alike; the valid batch still passes afterwards."""
    n, m = world.n, world.n // l
    rnd = random.Random(70 + l)
    rows = [rnd.randrange(3) for _ in range(96)]
    ks = rnd.sample(range(m), 96) if m >= 96 else [rnd.randrange(m) for _ in range(96)]
    ys, pf, g2 = world.items(l, rows, ks)
    V = k.verifier

    def both(rows_, ks_, ys_, pf_, g2_):
        a = world.verify(l, rows_, ks_, ys_, pf_, g2_)
        rp = V.compute_multiproof_r_powers(world.commitments, rows_, ks_, ys_, pf_, n)
        b = world.verify(l, rows_, ks_, ys_, pf_, g2_, r_powers=rp)
        assert a is b
        return a

    assert both(rows, ks, ys, pf, g2) is True
    bad = ys.copy()
    bad[40, l - 1] = k.fr.fr_from_int(k.fr.fr_to_int(bad[40, l - 1]) + 1)
    assert both(rows, ks, bad, pf, g2) is False                                # one y off by one
    i, j = 3, next(j for j in range(4, 96) if (rows[j], ks[j]) != (rows[3], ks[3]))
    swapped = list(pf)
    swapped[i], swapped[j] = swapped[j], swapped[i]
    assert both(rows, ks, ys, swapped, g2) is False                            # the proofs of two cosets swapped
    ks2 = list(ks)
    ks2[17] = (ks2[17] + 1) % m
    assert both(rows, ks2, ys, pf, g2) is False                                # a coset index off by one
    rows2 = list(rows)
    rows2[60] = (rows2[60] + 1) % 3
    assert both(rows2, ks, ys, pf, g2) is False                                # another polynomial's commitment
    wrong_g2 = k.helpers.g2_mul_generator(k.fr.fr_from_int(pow(TAU, 2 * l, R_)))
    assert both(rows, ks, ys, pf, wrong_g2) is False                           # [tau^(2l)]G2
    assert both(rows, ks, ys, pf, g2) is True


# ---- 8. degenerate inputs and the error table ------------------------------------------------------------------------------------
def test_degenerate_polynomials_and_empty_batch(k, world):
    """Known-tau SRS.  Constant polynomial: identity proofs; zero polynomial: identity commitment too.  count = 0 accepts."""
    n = world.n
    V = k.verifier
    const = k.PolynomialEvalForm(pyref.frs_to_mont([12345] * n))
    zero = k.PolynomialEvalForm(np.zeros((n, 4), np.uint64))
    for l in (1, 16):
        m = n // l
        g2 = world.at(l)[2]
        commitments, rows, ks, ys, pf = [], [], [], [], []
        for c, poly in enumerate((const, zero)):
            cm = world.kz.commit_eval_form(poly, world.srs)
            proofs = world.kz.compute_multiproofs(poly, world.srs, l)
            assert not proofs.any()
            assert k.fr.g1_is_identity(cm) == (c == 1)
            commitments.append(cm)
            co = world.kz.cosets(poly, l)
            for kk in (0, 1, m - 1):
                assert V.verify_multiproof(cm, proofs[kk], kk, co[kk], n, world.srs, g2) is True
                rows.append(c); ks.append(kk); ys.append(co[kk]); pf.append(proofs[kk])
        ys = np.stack(ys)
        assert world.verify(l, rows, ks, ys, pf, g2, commitments=commitments) is True
        assert world.verify(l, rows[::-1], ks, ys, pf, g2, commitments=commitments) is False    # the rows of the other polynomial
        assert world.verify(l, [], [], np.zeros((0, l, 4), np.uint64), [], g2) is True
        assert V.verify_multiproof_batch([], [], [], np.zeros((0, l, 4), np.uint64), [], n, world.srs, g2) is True


def test_error_table_in_the_documented_order_then_a_bit_exact_proof(k, world, test_srs_wire):
    """Known-tau SRS for the valid arguments; every error leaves the context usable (one bit-exact `compute_proof` at the end)."""
    L = k._lib
    lib = L.load()
    ctx = world.srs.ctx
    n, l = world.n, 16
    m = n // l
    z = world.kz.get_roots_of_unities()[3]
    before = world.kz.compute_proof(world.polys[0], z, world.srs)
    rows, ks = [0, 1, 2, 1], [5, 6, 7, m - 1]
    ys, pf, g2 = world.items(l, rows, ks)
    cm = np.ascontiguousarray(np.stack(world.commitments))
    pf = np.ascontiguousarray(np.stack(pf))
    ci, ki = np.array(rows, np.uint64), np.array(ks, np.uint64)
    ok = L.i32(7)
    lag = world.srs.lagrange(64)
    other_ctx = L.Context(0)
    other_srs = k.SRS(test_srs_wire[:64], order=64, ctx=other_ctx)
    small_srs = k.SRS(test_srs_wire[:8], order=8)

    def call(ctx_h=ctx.handle, srs_h=world.srs.handle, cm_=cm, M=3, ci_=ci, ki_=ki, ys_=ys, pf_=pf, count=4, n_=n, l_=l, g2_=g2, ok_=C.byref(ok)):
        P = lambda a: None if a is None else L.ptr(a)                          # noqa: E731
        return lib.kzg_verify_multiproof_batch(ctx_h, srs_h, P(cm_), M, P(ci_), P(ki_), P(ys_), P(pf_), count, n_, l_, None, P(g2_), ok_)

    assert call() == L.OK and ok.value == 1
    ok.value = 7
    for kw in (dict(ctx_h=None), dict(srs_h=None), dict(ok_=None), dict(cm_=None), dict(ci_=None), dict(ki_=None), dict(ys_=None), dict(pf_=None),
               dict(g2_=None), dict(srs_h=other_srs.handle), dict(srs_h=lag.handle)):
        assert call(**kw) == L.ERR_INVALID_ARG, kw
    assert call(n_=0) == L.ERR_NOT_POWER_OF_TWO and call(n_=96) == L.ERR_NOT_POWER_OF_TWO
    assert call(n_=1 << 25) == L.ERR_DOMAIN
    assert call(n_=1 << 25, l_=3) == L.ERR_DOMAIN                               # the domain before the chunk length
    for kw in (dict(n_=1, l_=1), dict(l_=3), dict(l_=0), dict(l_=n), dict(n_=16, l_=16)):
        assert call(**kw) == L.ERR_INVALID_ARG, kw
    assert call(srs_h=small_srs.handle) == L.ERR_SRS_CAPACITY_EXCEEDED          # l = 16 > 8 points
    assert call(srs_h=small_srs.handle, ki_=np.array([m, 0, 0, 0], np.uint64)) == L.ERR_SRS_CAPACITY_EXCEEDED     # ... before the indices
    assert call(ki_=np.array([5, 6, 7, m], np.uint64)) == L.ERR_INVALID_ARG
    assert call(ci_=np.array([0, 1, 3, 1], np.uint64)) == L.ERR_INVALID_ARG
    assert call(M=2) == L.ERR_INVALID_ARG
    huge = np.zeros((1 << 28) // l + 1, np.uint64)                              # never-touched zero pages: count * l > 2^28
    assert call(ci_=huge, ki_=huge, count=len(huge)) == L.ERR_TOO_LARGE
    del huge
    off = pf.copy()
    off[2, 4] ^= 1
    bad_g2 = g2.copy()
    bad_g2[0] ^= 1
    assert call(pf_=off) == L.ERR_G1_NOT_ON_CURVE
    assert call(pf_=off, g2_=bad_g2) == L.ERR_G1_NOT_ON_CURVE                   # a bad G1 point is reported before a bad G2 point
    offc = cm.copy()
    offc[1, 0] ^= 1
    assert call(cm_=offc) == L.ERR_G1_NOT_ON_CURVE
    assert call(g2_=bad_g2) == L.ERR_G2_TAU_NOT_ON_CURVE
    assert ok.value == 7                                                       # no error path writes the verdict
    # the Python surface maps them as _raise_for does
    V = k.verifier
    with pytest.raises(k.errors.NotOnCurveError, match="G1 point not on curve"):
        V.verify_multiproof_batch(world.commitments, rows, ks, ys, list(off), n, world.srs, g2)
    with pytest.raises(k.errors.NotOnCurveError, match="G2_TAU not on curve"):
        V.verify_multiproof(world.commitments[0], pf[0], ks[0], ys[0], n, world.srs, bad_g2)
    with pytest.raises(ValueError):                                            # KZG_ERR_INVALID_ARG, as everywhere in the library
        V.verify_multiproof(world.commitments[0], pf[0], m, ys[0], n, world.srs, g2)
    # kzg_coset_interpolate_rlc's own table
    one = pyref.frs_to_mont([1, 1, 1, 1])
    out = np.zeros((l, 4), np.uint64)
    rlc = lambda ctx_h=ctx.handle, ys_=ys, ki_=ki, w_=one, n_=n, l_=l, out_=out: lib.kzg_coset_interpolate_rlc(     # noqa: E731
        ctx_h, None if ys_ is None else L.ptr(ys_), None if ki_ is None else L.ptr(ki_), None if w_ is None else L.ptr(w_), 4, n_, l_,
        None if out_ is None else L.ptr(out_))
    assert rlc() == L.OK
    for kw in (dict(ctx_h=None), dict(ys_=None), dict(ki_=None), dict(w_=None), dict(out_=None), dict(l_=3), dict(l_=n),
               dict(ki_=np.array([5, 6, 7, m], np.uint64))):
        assert rlc(**kw) == L.ERR_INVALID_ARG, kw
    assert rlc(n_=96) == L.ERR_NOT_POWER_OF_TWO and rlc(n_=1 << 25) == L.ERR_DOMAIN
    assert call() == L.OK and ok.value == 1
    assert np.array_equal(world.kz.compute_proof(world.polys[0], z, world.srs), before)
    lag.close(); other_srs.close(); small_srs.close(); other_ctx.close()


# ---- 9. g2_tau_l = None: the mainnet [tau]_2 -------------------------------------------------------------------------------------
def test_g2_tau_l_none_is_the_mainnet_point(k, test_srs_wire, gettysburg, golden_dir):
    """The reference's 3 000-point test SRS, whose tau is NOT the mainnet one: the golden proofs of kzg.proof.eq.input are rejected by
    `verify_proof(.., None)` and by `verify_multiproof(l = 1, None)` alike; both accept (identity commitment, identity proof, y = 0)."""
    srs = k.SRS(test_srs_wire, order=3000)
    blob = k.Blob.from_raw_data(gettysburg)
    kz = k.KZG.new()
    kz.calculate_and_store_roots_of_unity(len(blob))
    poly = blob.to_polynomial_eval_form()
    n = len(poly)
    commitment = kz.commit_eval_form(poly, srs)
    V = k.verifier
    lines = [ln.strip().split(",") for ln in open(os.path.join(golden_dir, "kzg.proof.eq.input")) if ln.strip()]
    for idx, x, y in lines[:4]:
        idx = int(idx)
        proof = pyref.point_to_wire((int(x), int(y)))
        value, z = poly.get_evalualtion(idx), kz.get_nth_root_of_unity(idx)
        a = V.verify_proof(commitment, proof, value, z, None)
        b = V.verify_multiproof(commitment, proof, idx, [value], n, srs, None)
        assert a is False and b is False
    ident, zero = np.zeros(8, np.uint64), np.zeros(4, np.uint64)
    assert V.verify_proof(ident, ident, zero, kz.get_nth_root_of_unity(1), None) is True
    assert V.verify_multiproof(ident, ident, 1, [zero], n, srs, None) is True
    assert V.verify_multiproof_batch([ident], [0, 0], [1, 2], np.zeros((2, 1, 4), np.uint64), [ident, ident], n, srs, None) is True
    srs.close()


# ---- 10. two threads on one context, a second context beside them ---------------------------------------------------------------
def test_threads_and_contexts_at_once(k, world):
    """Known-tau SRS on every context.  Verdicts of valid and faulted batches are unchanged when the calls run concurrently."""
    l = 16
    m = world.n // l
    rnd = random.Random(1001)
    rows = [rnd.randrange(3) for _ in range(128)]
    ks = [rnd.randrange(m) for _ in range(128)]
    ys, pf, g2 = world.items(l, rows, ks)
    bad = ys.copy()
    bad[9, 0] = k.fr.fr_from_int(1)
    ctx_a, ctx_b = k._lib.Context(0), k._lib.Context(0)
    wa, wb = World(k, ctx_a), World(k, ctx_b)                                   # same polynomials: same commitments and proofs
    assert all(np.array_equal(a, b) for a, b in zip(wa.commitments, world.commitments))
    z = wa.kz.get_roots_of_unities()[7]
    want_proof = world.kz.compute_proof(world.polys[0], z, world.srs)
    errors, results = [], {}

    def run(name, fn):
        try:
            results[name] = fn()
        except Exception as e:                                                  # reported below
            errors.append((name, repr(e)))

    def batches(w):
        return lambda: [(w.verify(l, rows, ks, ys, pf, g2), w.verify(l, rows, ks, bad, pf, g2)) for _ in range(4)]

    def singles():
        out = []
        for i in range(6):
            out.append((k.verifier.verify_multiproof(wa.commitments[rows[i]], pf[i], ks[i], ys[i], wa.n, wa.srs, g2),
                        wa.kz.compute_proof(wa.polys[0], z, wa.srs)))
        return out

    ts = [threading.Thread(target=run, args=(nm, fn)) for nm, fn in (("a", batches(wa)), ("singles", singles), ("b", batches(wb)))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert results["a"] == [(True, False)] * 4 and results["b"] == [(True, False)] * 4
    for okv, proof in results["singles"]:
        assert okv is True and np.array_equal(proof, want_proof)
    wa.srs.close(); wb.srs.close()
    ctx_a.close(); ctx_b.close()


# ---- 11. the bound-checked build runs tests 5-8 with every site counter at 0 ----------------------------------------------------
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
WORKLOAD = ["tests/test_gpu_multiproof_verify.py::" + t for t in (
    "test_coset_interpolate_rlc_is_bit_equal_to_big_integers", "test_coset_interpolate_rlc_equal_indices_and_item_order",
    "test_coset_interpolate_rlc_at_the_largest_domain_without_an_n_sized_table", "test_every_proof_of_compute_multiproofs_verifies",
    "test_a_single_fault_rejects_the_batch", "test_degenerate_polynomials_and_empty_batch",
    "test_error_table_in_the_documented_order_then_a_bit_exact_proof")]


def test_bound_checked_build_keeps_every_precondition():
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": WORKLOAD}], capture_output=True, text=True, timeout=1500,
                         env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "PYTEST_RC 0" in out, (out[-3000:], res.stderr[-2000:])
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert sites
    fired = {int(s[1]): int(s[2]) for s in sites if int(s[2])}
    assert not fired, fired
