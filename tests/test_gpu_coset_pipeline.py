"""-m gpu: the three routes to the batch equation of coset proofs -- `kzg_verify_multiproof_batch` (wire words),
`kzg_verify_multiproof_batch_bytes` (serialized items) and the summed pairs of `kzg_coset_group_sums` checked with `kzg_pairings_verify` --
must agree, through the public entries only: on clean and corrupted batches with the transcript on the host and on the device, after a
larger call has left its data in the context's buffers, with identity points and repeated items, on the error order at the last proof and
the last commitment, and while a `kzg_msm_g1_srs_begin` holds slot 0.  A known-tau SRS of 4 096 points, as tests/test_gpu_coset_bytes.py."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import pyref

pytestmark = pytest.mark.gpu
R_ = pyref.R_
TAU = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/coset-pipeline/v1").digest(), "big") % R_
N_DOMAIN = 4096
SHAPES = [(1, 1, 1), (1, 257, 3), (16, 3, 5), (64, 257, 1)]                             # (l, count, M); the third leaves rows unused


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


class World:
    """Five commitments on a known-tau SRS: three random polynomials of 4 096 evaluations, a constant one (identity proofs) and the zero
    polynomial (identity commitment too); per chunk length their proofs and cosets."""

    def __init__(self, k):
        self.k, self.n = k, N_DOMAIN
        self.srs = k.SRS.generate(TAU, self.n)
        self.kz = k.KZG.new()
        self.kz.calculate_and_store_roots_of_unity(self.n * 32)
        rnd = random.Random(777)
        self.polys = [k.PolynomialEvalForm(pyref.frs_to_mont([rnd.randrange(R_) for _ in range(self.n)])) for _ in range(3)]
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

    def batch(self, l, rows, ks, M):
        proofs, cosets, g2 = self.at(l)
        ys = np.ascontiguousarray(np.stack([cosets[c][kk] for c, kk in zip(rows, ks)]))
        pf = np.ascontiguousarray(np.stack([proofs[c][kk] for c, kk in zip(rows, ks)]))
        return Batch(self, l, list(rows), list(ks), ys, pf, list(self.commitments[:M]), g2)

    def random_batch(self, l, count, M, seed=0):
        rnd = random.Random(1000 * l + 10 * count + M + seed)
        rows = [rnd.randrange(min(M, 3)) for _ in range(count)]
        ks = [rnd.randrange(self.n // l) for _ in range(count)]
        ks[0] = self.n // l - 1
        return self.batch(l, rows, ks, M)


class Batch:
    def __init__(self, world, l, rows, ks, ys, pf, cms, g2):
        self.w, self.l, self.rows, self.ks, self.ys, self.pf, self.cms, self.g2 = world, l, rows, ks, ys, pf, cms, g2

    def replace(self, **kw):
        b = Batch(self.w, self.l, list(self.rows), list(self.ks), self.ys.copy(), self.pf.copy(), list(self.cms), self.g2)
        for name, v in kw.items():
            setattr(b, name, v)
        return b

    def with_bad_value(self, item, j):
        k = self.w.k
        ys = self.ys.copy()
        ys[item, j] = k.fr.fr_from_int((k.fr.fr_to_int(ys[item, j]) + 1) % R_)
        return self.replace(ys=ys)

    # ---- the three routes ------------------------------------------------------------------------------------------------------------
    def words(self, r_powers=None, g2=None):
        V, w = self.w.k.verifier, self.w
        return V.verify_multiproof_batch(self.cms, self.rows, self.ks, self.ys, list(self.pf), w.n, w.srs, self.g2 if g2 is None else g2, r_powers=r_powers)

    def bytes_(self, r_powers=None, g2=None):
        k, w = self.w.k, self.w
        ys_be, pf_be = k.verifier.encode_coset_items(self.ys, self.pf)
        cm_be = k.helpers.compress_g1_be(np.stack(self.cms))
        return k.verifier.verify_multiproof_batch_bytes(cm_be, self.rows, self.ks, ys_be, pf_be, w.n, self.l, w.srs, self.g2 if g2 is None else g2,
                                                        r_powers=r_powers, return_r_powers=True)

    def group_sums(self, r_powers=None):
        V, w = self.w.k.verifier, self.w
        return V.coset_group_sums(self.cms, self.rows, self.ks, self.ys, list(self.pf), w.n, w.srs, r_powers)            # one group per commitment row

    def summed(self, r_powers=None):
        V, H = self.w.k.verifier, self.w.k.helpers
        lhs, _, rhs, _ = self.group_sums(r_powers)
        total = lambda pts: pyref.point_to_wire(_sum([pyref.point_from_wire(p) for p in pts]))      # noqa: E731
        return V.pairings_verify(total(lhs), self.g2, total(rhs), H.g2_generator())

    def verdicts(self):
        return self.words(), self.bytes_()[0], self.summed()

    def weights(self):
        return self.w.k.verifier.compute_multiproof_r_powers(self.cms, self.rows, self.ks, self.ys, list(self.pf), self.w.n)


def _sum(pts):
    acc = None
    for p in pts:
        acc = pyref.ec_add(acc, p)
    return acc


@pytest.fixture(scope="module")
def world(k):
    return World(k)


# ---- 1. agreement across the three routes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2], ids=["host transcript", "device transcript"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "l%d-count%d-M%d" % s)
def test_three_routes_agree(k, world, shape, mode):
    l, count, M = shape
    b = world.random_batch(l, count, M)
    want = b.weights()                                                                  # the host transcript entry
    ctx = world.srs.ctx
    ctx.set_transcript_device(mode)
    try:
        # a clean batch: all accept, the weights agree
        assert b.words() is True
        ok, rp = b.bytes_()
        assert ok is True and np.array_equal(rp, want)
        assert np.array_equal(k.verifier.compute_multiproof_r_powers(b.cms, b.rows, b.ks, b.ys, list(b.pf), world.n, ctx=ctx, device=True), want)
        derived, supplied = b.group_sums(), b.group_sums(want)
        assert all(np.array_equal(x, y) for x, y in zip(derived, supplied))             # derived weights are the transcript's: supplying them changes no bit
        assert b.summed() is True
        assert b.words(r_powers=want) is True and b.bytes_(r_powers=want)[0] is True
        # one value corrupted
        assert b.with_bad_value(count - 1, l - 1).verdicts() == (False, False, False)
        # a proof swapped for another valid point
        pf = b.pf.copy()
        pf[0] = world.commitments[1]
        assert b.replace(pf=pf).verdicts() == (False, False, False)
        # the last item's commitment index changed (with one row there is no other index)
        if M > 1:
            rows = list(b.rows)
            rows[-1] = (rows[-1] + 1) % M
            assert b.replace(rows=rows).verdicts() == (False, False, False)
    finally:
        ctx.set_transcript_device(0)


# ---- 2. no stale data after workspace reuse ----------------------------------------------------------------------------------------------
def test_a_smaller_call_reads_nothing_a_larger_one_left(k, world):
    l = 16
    big, three, mid, one = (world.random_batch(l, c, 3, seed=s) for c, s in ((257, 1), (3, 2), (65, 3), (1, 4)))
    big2 = world.random_batch(l, 257, 3, seed=5)
    assert big.words() is True
    assert three.bytes_()[0] is True
    assert mid.summed() is True
    assert one.words() is True
    assert big2.bytes_()[0] is True
    assert one.bytes_()[0] is True
    bad = one.with_bad_value(0, 3)
    assert big.words() is True and bad.words() is False                                 # N = 1 behind N = 257, on either route
    assert big2.bytes_()[0] is True and bad.bytes_()[0] is False
    assert big.words() is True and bad.bytes_()[0] is False
    assert big2.bytes_()[0] is True and bad.words() is False
    assert mid.summed() is True and bad.summed() is False
    assert one.verdicts() == (True, True, True)


# ---- 3. identities and repeated items ----------------------------------------------------------------------------------------------------
def test_identity_points_and_a_repeated_item(k, world):
    l, m = 16, N_DOMAIN // 16
    rows = [3, 0, 4, 1, 0, 3]                                                           # 3: identity proofs; 4: identity commitment, zero values
    ks = [5, 9, m - 1, 0, 9, 5]                                                         # items 1 and 4, 0 and 5: the same item twice
    b = world.batch(l, rows, ks, 5)
    assert not b.cms[4].any() and not b.pf[0].any() and not b.pf[2].any() and not b.ys[2].any()
    assert b.verdicts() == (True, True, True)
    assert np.array_equal(b.bytes_()[1], b.weights())
    assert b.with_bad_value(4, 0).verdicts() == (False, False, False)                   # one of the two copies


# ---- 4. errors at the edges of the layout proofs | proofs | commitments --------------------------------------------------------------------
def _off_curve(point):
    p = point.copy()
    p[4] ^= 1                                                                           # y +- 1 in Montgomery form: no point of that x
    return p


def test_off_curve_points_at_the_last_proof_and_the_last_commitment(k, world):
    G = k.errors.NotOnCurveError
    b = world.random_batch(16, 257, 3, seed=11)
    bad_g2 = b.g2.copy()
    bad_g2[0] ^= 1
    pf = b.pf.copy()
    pf[256] = _off_curve(pf[256])
    cms = list(b.cms)
    cms[2] = _off_curve(cms[2])
    for broken in (b.replace(pf=pf), b.replace(cms=cms), b.replace(pf=pf, cms=cms)):
        for g2 in (None, bad_g2):                                                       # ... and before a G2 point off the twist
            with pytest.raises(G, match="G1 point not on curve"):
                broken.words(g2=g2)
        with pytest.raises(G, match="G1 point not on curve"):
            broken.group_sums()
    with pytest.raises(G, match="G2_TAU not on curve"):
        b.words(g2=bad_g2)
    with pytest.raises(G, match="G2_TAU not on curve"):
        b.bytes_(g2=bad_g2)
    assert b.verdicts() == (True, True, True)                                           # the context is usable after every error


def test_a_begin_in_flight_on_slot_0_is_refused_with_each_entrys_text(k, world):
    L = k._lib
    lib, ctx = L.load(), world.srs.ctx
    b = world.random_batch(16, 257, 3, seed=12)
    sc = np.ascontiguousarray(pyref.frs_to_mont(list(range(1, 65))))
    xy, inf = np.zeros(8, np.uint64), C.c_uint8(0)
    assert lib.kzg_msm_g1_srs_begin(ctx.handle, world.srs.handle, 0, L.ptr(sc), 64, 0) == L.OK
    try:
        with pytest.raises(ValueError, match="invalid argument"):
            b.words()
        assert ctx.last_error() == "a kzg_*_begin on slot 0 is still in flight: call kzg_msm_g1_srs_end(ctx, 0, ..) first"
        with pytest.raises(ValueError, match="invalid argument"):
            b.bytes_()
        assert ctx.last_error() == "a kzg_*_begin on slot 0 is still in flight: call its end first"
    finally:
        assert lib.kzg_msm_g1_srs_end(ctx.handle, 0, L.ptr(xy), C.byref(inf), None) == L.OK
    assert pyref.point_from_wire(xy) == pyref.ec_mul(sum(i * pow(TAU, i - 1, R_) for i in range(1, 65)), (1, 2))          # the MSM in flight was not disturbed
    assert b.words() is True and b.bytes_()[0] is True
