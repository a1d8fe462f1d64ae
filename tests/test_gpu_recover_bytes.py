"""-m gpu: the retriever's half on serialized chunks -- `kzg_recover_from_cosets_batch_bytes` (values decoded where the scatter kernel
loads them, rows encoded where the last kernel stores them) and `kzg_retrieve_blobs_bytes` (verify, then recover, values uploaded once).

The reference everywhere is the three-call composition a caller had before: `kzg_coset_items_decode_be`, `kzg_recover_from_cosets_batch`,
`kzg_coset_items_encode_be`, compared byte for byte and flag for flag; behind it tests/recover_ref.py, which also pins one fixed seed by
a SHA-256 digest (PIN) that neither the composition nor the new entry had a hand in.  Shapes: (16, 1), (16, 8) and (2048, 16), one size
above 2^10 where the transforms' workspace changes; count in {m / 2, m - 1, m}; items shuffled; both output forms and coefficient rows
cut to out_len = degree_bound < n; B in {1, 3}, B = 5 in three groups; index rows 1 and B; the values 0, 1 and r - 1 among the inputs."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pyref
import recover_ref
from coset_bytes_ref import P
from pyref import R_

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
u8p = C.POINTER(C.c_uint8)
i32p = C.POINTER(C.c_int32)
TAU = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/recover-bytes/v1").digest(), "big") % R_
# sha256 over, per blob, the 64 coefficients then the 64 evaluations (32 big-endian bytes each) tests/recover_ref.py gives for the inputs
# of pin_inputs(): computed once from recover_ref alone
PIN = "35b3fa566226b2b939127aa8c5be3c04c8024c27a11aafa219c29274e0aeece8"
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


def be(ints):
    return b"".join(int(v).to_bytes(32, "big") for v in ints)


def random_values_be(B, count, l, seed):
    """B x count x l canonical values as bytes; the first three of the call are 0, 1 and r - 1 (as far as there is room)."""
    rnd = random.Random(seed)
    vals = [rnd.randrange(R_) for _ in range(B * count * l)]
    edge = (0, 1, R_ - 1)[:len(vals)]
    vals[:len(edge)] = edge
    return be(vals)


def random_rows(B, m, count, seed):
    rnd = random.Random(seed)
    return np.array([rnd.sample(range(m), count) for _ in range(B)], dtype=np.uint64)


def composition(k, ctx, ys_be, idx, B, count, n, l, bound, form, out_len=0):
    """decode call, words recovery, host encode: (bytes, flags)."""
    L = k._lib
    ys, _ = k.verifier.decode_coset_items(ys_be, None, l, ctx=ctx)
    ys = np.ascontiguousarray(ys.reshape(B, count, l, 4))
    idx = np.ascontiguousarray(idx, dtype=np.uint64)
    rows = out_len or n
    out = np.zeros((B, rows, 4), dtype=np.uint64)
    fl = np.full(B, -1, dtype=np.int32)
    rc = L.load().kzg_recover_from_cosets_batch(ctx.handle, L.ptr(ys), L.ptr(idx), 1 if idx.ndim == 1 else B, B, count, n, l, bound, form, out_len, L.ptr(out),
                                                fl.ctypes.data_as(i32p))
    assert rc == 0, rc
    return k.verifier.encode_coset_items(out.reshape(B * rows, 1, 4), None)[0], fl


def fused(k, ctx, ys_be, idx, B, count, n, l, bound, form, out_len=0):
    """The C-ABI entry: (status, bytes, flags, bad index); outputs start from a sentinel."""
    L = k._lib
    buf = np.frombuffer(ys_be, np.uint8)
    idx = np.ascontiguousarray(idx, dtype=np.uint64)
    out = np.full(B * (out_len or n) * 32, SENTINEL, dtype=np.uint8)
    fl = np.full(B, -1, dtype=np.int32)
    bad = C.c_uint64(1 << 40)
    rc = L.load().kzg_recover_from_cosets_batch_bytes(ctx.handle, buf.ctypes.data_as(u8p), L.ptr(idx), 1 if idx.ndim == 1 else B, B, count, n, l, bound, form, out_len,
                                                      out.ctypes.data_as(u8p), fl.ctypes.data_as(i32p), C.byref(bad))
    return rc, out.tobytes(), fl, bad.value


def counts(m):
    return sorted({max(1, m // 2), m - 1, m} - {0})


# ---- 1. bit identity with the composition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n,l", [(16, 1), (16, 8), (2048, 16)])
def test_bit_identity_with_the_three_call_composition(k, n, l, B):
    ctx = k.default_context()
    m = n // l
    for count in counts(m):
        ys_be = random_values_be(B, count, l, "%d/%d/%d/%d" % (n, l, B, count))
        rows = random_rows(B, m, count, n + l + B + count)                              # shuffled item order
        bound = max(1, count * l // 2)
        for idx in (rows, rows[0]):
            for form, deg, out_len in ((1, 0, 0), (0, 0, 0), (0, bound, bound)):       # evaluations, coefficients, coefficients cut to the bound < n
                want, want_flags = composition(k, ctx, ys_be, idx, B, count, n, l, deg, form, out_len)
                rc, got, flags, _ = fused(k, ctx, ys_be, idx, B, count, n, l, deg, form, out_len)
                assert rc == 0 and got == want, (count, form, out_len, idx.ndim)
                assert np.array_equal(flags, want_flags)


def test_three_groups_give_the_same_bytes(k):
    L = k._lib
    ctx = L.Context(0)
    n, l, B = 2048, 16, 5
    m = n // l
    count = m - 1
    per = k.helpers.recover_batch_info(B, count, n, l)["blob_bytes"]
    assert k.helpers.recover_batch_info(B, count, n, l, 0, 2 * per)["groups"] >= 3
    ys_be = random_values_be(B, count, l, "groups")
    rows = random_rows(B, m, count, 55)
    for idx in (rows, rows[3]):
        for form, deg, out_len in ((1, 0, 0), (0, 0, 0), (0, 1000, 1000)):
            ctx.set_recover_group_bytes(0)
            want, want_flags = composition(k, ctx, ys_be, idx, B, count, n, l, deg, form, out_len)
            ctx.set_recover_group_bytes(2 * per)
            rc, got, flags, _ = fused(k, ctx, ys_be, idx, B, count, n, l, deg, form, out_len)
            assert rc == 0 and got == want and np.array_equal(flags, want_flags)
    ctx.close()


# ---- 2. one seed pinned by tests/recover_ref.py alone ------------------------------------------------------------------------------------
def pin_inputs():
    n, l, count, B = 64, 4, 9, 2
    rnd = random.Random("recover-bytes/pin/v1")
    ks, ys = [], []
    for _ in range(B):
        ks.append(rnd.sample(range(n // l), count))
        ys.append([[rnd.randrange(R_) for _ in range(l)] for _ in range(count)])
    return n, l, count, B, ks, ys


def test_the_reference_digest_is_reproduced(k):
    n, l, count, B, ks, ys = pin_inputs()
    h = hashlib.sha256()
    for b in range(B):
        coeffs, consistent = recover_ref.recover(n, l, ks[b], ys[b], count * l)
        assert consistent
        h.update(be(coeffs) + be(recover_ref.fft([int(c) for c in coeffs])))
    assert h.hexdigest() == PIN                                                         # the pin is the reference's, whatever the library does
    ctx = k.default_context()
    ys_be = be(v for blob in ys for item in blob for v in item)
    idx = np.array(ks, dtype=np.uint64)

    def digest(call):
        c = call(k, ctx, ys_be, idx, B, count, n, l, 0, 0)
        e = call(k, ctx, ys_be, idx, B, count, n, l, 0, 1)
        bc, be_ = (c[0], e[0]) if call is composition else (c[1], e[1])
        return hashlib.sha256(b"".join(bc[b * n * 32:(b + 1) * n * 32] + be_[b * n * 32:(b + 1) * n * 32] for b in range(B))).hexdigest()

    assert digest(composition) == PIN                                                   # the route a caller had: independent of the new symbols
    assert digest(fused) == PIN                                                         # the new entry


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------
def with_value(ys_be, at, v):
    b = bytearray(ys_be)
    b[32 * at:32 * at + 32] = int(v).to_bytes(32, "big")
    return bytes(b)


@pytest.mark.parametrize("bad_value", [R_, R_ + 1, 2 ** 256 - 1])
def test_a_value_not_below_r_is_refused_with_its_item(k, bad_value):
    L = k._lib
    ctx = L.Context(0)
    n, l, B, count = 64, 4, 3, 8
    rows = random_rows(B, n // l, count, 9)
    good = random_values_be(B, count, l, "refusals")
    want, want_flags = composition(k, ctx, good, rows, B, count, n, l, 0, 1)
    item = 1 * count + 5                                                                # an item of blob 1; the blob's other items are fine
    for j in (0, l - 1):
        rc, _, _, bad = fused(k, ctx, with_value(good, item * l + j, bad_value), rows, B, count, n, l, 0, 1)
        assert (rc, bad) == (L.ERR_DESERIALIZE, item)
        assert "value of item %d" % item in ctx.last_error()
    # two bad values in one call: the smaller item is reported
    two = with_value(with_value(good, (2 * count + 1) * l + 2, bad_value), (0 * count + 6) * l + 3, bad_value)
    rc, _, _, bad = fused(k, ctx, two, rows, B, count, n, l, 0, 0)
    assert (rc, bad) == (L.ERR_DESERIALIZE, 6)
    # r - 1 in the same place decodes; the context is as usable as before
    rc, got, flags, _ = fused(k, ctx, good, rows, B, count, n, l, 0, 1)
    assert rc == 0 and got == want and np.array_equal(flags, want_flags)
    kz = k.KZG.new(ctx)
    with pytest.raises(k.errors.DeserializationError, match=r"value of item %d\b" % item):
        kz.recover_from_cosets_batch_bytes(rows, with_value(good, item * l, bad_value), n, l)
    out, consistent = kz.recover_from_cosets_batch_bytes(rows, good, n, l)
    assert out == want and consistent.tolist() == [bool(f) for f in want_flags]
    ctx.close()


def test_a_bad_value_in_the_last_of_three_groups(k):
    L = k._lib
    ctx = L.Context(0)
    n, l, B = 2048, 16, 5
    m = n // l
    count = m // 2
    per = k.helpers.recover_batch_info(B, count, n, l)["blob_bytes"]
    ctx.set_recover_group_bytes(2 * per)
    assert k.helpers.recover_batch_info(B, count, n, l, 0, 2 * per)["groups"] == 3
    rows = random_rows(B, m, count, 77)
    good = random_values_be(B, count, l, "last group")
    item = 4 * count + count - 1                                                        # the last item of the last blob: group 2
    rc, _, _, bad = fused(k, ctx, with_value(good, item * l + 7, R_), rows, B, count, n, l, 0, 0)
    assert (rc, bad) == (L.ERR_DESERIALIZE, item)
    # ... and one in the first group beside it: the first group's is the smallest of the call
    both = with_value(with_value(good, item * l + 7, R_), (1 * count + 3) * l, R_ + 5)
    rc, _, _, bad = fused(k, ctx, both, rows, B, count, n, l, 0, 0)
    assert (rc, bad) == (L.ERR_DESERIALIZE, count + 3)
    want, want_flags = composition(k, ctx, good, rows, B, count, n, l, 0, 0)
    rc, got, flags, _ = fused(k, ctx, good, rows, B, count, n, l, 0, 0)
    assert rc == 0 and got == want and np.array_equal(flags, want_flags)
    ctx.close()


def test_the_table_of_the_words_entry_then_the_cap(k):
    L = k._lib
    ctx = k.default_context()
    n, l, B, count = 64, 4, 3, 5
    rows = random_rows(B, n // l, count, 3)
    ys_be = random_values_be(B, count, l, "table")
    assert fused(k, ctx, ys_be, rows, B, count, 96, l, 0, 0)[0] == L.ERR_NOT_POWER_OF_TWO
    assert fused(k, ctx, ys_be, rows, B, count, n, 3, 0, 0)[0] == L.ERR_INVALID_ARG
    dup = rows.copy(); dup[1, 4] = dup[1, 0]
    assert fused(k, ctx, ys_be, dup, B, count, n, l, 0, 0)[0] == L.ERR_INVALID_ARG
    assert fused(k, ctx, ys_be, rows, B, count, n, l, count * l + 1, 0)[0] == L.ERR_INVALID_ARG
    rc, out, flags, _ = fused(k, ctx, ys_be, rows, B, count, n, l, 0, 1, n - 1)
    assert rc == L.ERR_INVALID_ARG and set(out) == {SENTINEL} and (flags == -1).all()


# ---- 4. kzg_retrieve_blobs_bytes ---------------------------------------------------------------------------------------------------------------
class World:
    """B = 3 polynomials of d = 64 coefficients on a known-tau SRS, encoded at rate 1/2 (n = 128); per chunk length every coset and proof."""

    def __init__(self, k):
        self.k, self.d, self.n, self.B = k, 64, 128, 3
        self.srs = k.SRS.generate(TAU, self.n)
        self.kz = k.KZG.new()
        rnd = random.Random(2718)
        self.coeffs = [[rnd.randrange(R_) for _ in range(self.d)] for _ in range(self.B)]
        self.polys = [k.PolynomialCoeffForm(pyref.frs_to_mont(c)) for c in self.coeffs]
        self.commitments_be = k.helpers.compress_g1_be(np.stack([self.kz.commit_coeff_form(p, self.srs) for p in self.polys]))
        self._by_l = {}

    def at(self, l):
        if l not in self._by_l:
            ys, proofs = self.kz.encode_cosets_batch(self.polys, self.srs, self.n, l)
            g2 = self.k.helpers.g2_mul_generator(self.k.fr.fr_from_int(pow(TAU, l, R_)))
            self._by_l[l] = (ys, proofs, g2)
        return self._by_l[l]

    def chunks(self, l, seed=0, blobs=None):
        """m / 2 cosets per blob, different per blob, shuffled: (rows, ys_be, proofs_be, g2)"""
        ys, proofs, g2 = self.at(l)
        B = blobs or self.B
        m = self.n // l
        rows = random_rows(B, m, m // 2, 31 * l + seed)
        pick = rows.astype(np.int64)
        sel_y = np.ascontiguousarray(np.stack([ys[b][pick[b]] for b in range(B)])).reshape(-1, l, 4)
        sel_p = np.ascontiguousarray(np.stack([proofs[b][pick[b]] for b in range(B)])).reshape(-1, 8)
        ys_be, pf_be = self.k.verifier.encode_coset_items(sel_y, sel_p)
        return rows, ys_be, pf_be, g2


@pytest.fixture(scope="module")
def world(k):
    return World(k)


def retrieve(k, w, rows, ys_be, pf_be, g2, l, bound=0, form=0, out_len=0, r_powers=None, commitments_be=None, blobs=None):
    """The C entry itself: (rc, ok, bytes, flags, bad index, bad array); the outputs start from a sentinel."""
    L = k._lib
    B = blobs or w.B
    cm = np.frombuffer(commitments_be or w.commitments_be[:32 * B], np.uint8)
    yb, pb = np.frombuffer(ys_be, np.uint8), np.frombuffer(pf_be, np.uint8)
    idx = np.ascontiguousarray(rows, dtype=np.uint64)
    count = idx.shape[-1]
    out = np.full(B * (out_len or w.n) * 32, SENTINEL, dtype=np.uint8)
    fl = np.full(B, -1, dtype=np.int32)
    ok, bad, arr = C.c_int32(-1), C.c_uint64(1 << 40), C.c_int32(-1)
    rp = None if r_powers is None else np.ascontiguousarray(r_powers, dtype=np.uint64)
    rc = L.load().kzg_retrieve_blobs_bytes(L.default_context().handle, w.srs.handle, cm.ctypes.data_as(u8p), L.ptr(idx), 1 if idx.ndim == 1 else B,
                                           yb.ctypes.data_as(u8p), pb.ctypes.data_as(u8p), B, count, w.n, l, bound, form, out_len, None if rp is None else L.ptr(rp),
                                           L.ptr(np.ascontiguousarray(g2, dtype=np.uint64)), C.byref(ok), out.ctypes.data_as(u8p), fl.ctypes.data_as(i32p),
                                           C.byref(bad), C.byref(arr))
    return rc, ok.value, out.tobytes(), fl, bad.value, arr.value


def verifier_items(w, rows):
    B, count = rows.shape
    return [b for b in range(B) for _ in range(count)], [int(v) for v in rows.reshape(-1)]


@pytest.mark.parametrize("l", [1, 16])
def test_retrieve_accepts_and_recovers_the_blobs(k, world, l):
    w = world
    rows, ys_be, pf_be, g2 = w.chunks(l)
    want = b"".join(be(c) for c in w.coeffs)
    rc, ok, got, flags, _, _ = retrieve(k, w, rows, ys_be, pf_be, g2, l, bound=w.d, form=0, out_len=w.d)
    assert (rc, ok) == (0, 1) and got == want and flags.tolist() == [1, 1, 1]      # the coefficient rows are the original coefficients
    # the outputs are those of kzg_recover_from_cosets_batch_bytes on the same values, in both forms
    ctx = k.default_context()
    count = rows.shape[1]
    for form in (0, 1):
        rc, ok, got, flags, _, _ = retrieve(k, w, rows, ys_be, pf_be, g2, l, form=form)
        rc2, want2, flags2, _ = fused(k, ctx, ys_be, rows, w.B, count, w.n, l, 0, form)
        assert (rc, ok, rc2) == (0, 1, 0) and got == want2 and np.array_equal(flags, flags2)
    # supplied weights and derived weights: the same verdict; the derived ones are those of the bytes transcript
    ci, ki = verifier_items(w, rows)
    weights = k.verifier.compute_multiproof_r_powers_bytes(w.commitments_be, ci, ki, ys_be, pf_be, w.n, l)
    ok_v, used = k.verifier.verify_multiproof_batch_bytes(w.commitments_be, ci, ki, ys_be, pf_be, w.n, l, w.srs, g2, return_r_powers=True)
    assert ok_v and np.array_equal(used, weights)
    rc, ok, got, flags, _, _ = retrieve(k, w, rows, ys_be, pf_be, g2, l, bound=w.d, out_len=w.d, r_powers=weights)
    assert (rc, ok) == (0, 1) and got == want and flags.all()
    # a degree bound below the true degree: accepted, not consistent
    rc, ok, got, flags, _, _ = retrieve(k, w, rows, ys_be, pf_be, g2, l, bound=w.d - 1, out_len=w.d)
    assert (rc, ok) == (0, 1) and got == want and flags.tolist() == [0, 0, 0]
    # the Python surface
    ok, polys, consistent = k.verifier.retrieve_blobs_bytes(w.commitments_be, rows, ys_be, pf_be, w.n, l, w.srs, g2, degree_bound=w.d, eval_form=False, out_len=w.d)
    assert ok is True and polys == want and consistent.all()


@pytest.mark.parametrize("l", [1, 16])
def test_retrieve_refuses_without_touching_the_outputs(k, world, l):
    w = world
    L = k._lib
    rows, ys_be, pf_be, g2 = w.chunks(l, seed=1)
    count = rows.shape[1]
    ci, ki = verifier_items(w, rows)
    flipped = bytearray(ys_be)
    flipped[32 * (count * l + 2) + 31] ^= 1                                            # a value of blob 1, still below r
    swapped = bytearray(pf_be)
    swapped[0:32], swapped[32:64] = pf_be[32:64], pf_be[0:32]                           # two valid points, each on the wrong item
    for ys_x, pf_x in ((bytes(flipped), pf_be), (ys_be, bytes(swapped))):
        rc, ok, out, flags, _, _ = retrieve(k, w, rows, ys_x, pf_x, g2, l, bound=w.d, out_len=w.d)
        assert (rc, ok) == (0, 0) and set(out) == {SENTINEL} and (flags == -1).all()
        assert k.verifier.verify_multiproof_batch_bytes(w.commitments_be, ci, ki, ys_x, pf_x, w.n, l, w.srs, g2) is False
        assert k.verifier.retrieve_blobs_bytes(w.commitments_be, rows, ys_x, pf_x, w.n, l, w.srs, g2) == (False, None, None)
    # what does not decode: the verifier's status, array and index
    item = 2 * count + 1
    bad_value = with_value(ys_be, item * l + (l - 1), R_)
    bad_proof = bytearray(pf_be); bad_proof[32 * item] &= 0x3F                          # flag bits 0b00
    bad_commitment = bytearray(w.commitments_be); bad_commitment[32:64] = P.to_bytes(32, "big")
    bad_commitment[32] |= 0x80                                                          # x = p under a valid flag
    for ys_x, pf_x, cm_x, arr, index in ((bad_value, pf_be, None, 2, item), (ys_be, bytes(bad_proof), None, 1, item), (ys_be, pf_be, bytes(bad_commitment), 0, 1)):
        rc, ok, out, flags, bad, bad_arr = retrieve(k, w, rows, ys_x, pf_x, g2, l, bound=w.d, out_len=w.d, commitments_be=cm_x)
        assert (rc, bad, bad_arr) == (L.ERR_DESERIALIZE, index, arr) and set(out) == {SENTINEL} and (flags == -1).all()
        with pytest.raises(k.errors.DeserializationError) as e_new:
            k.verifier.retrieve_blobs_bytes(cm_x or w.commitments_be, rows, ys_x, pf_x, w.n, l, w.srs, g2)
        with pytest.raises(k.errors.DeserializationError) as e_old:
            k.verifier.verify_multiproof_batch_bytes(cm_x or w.commitments_be, ci, ki, ys_x, pf_x, w.n, l, w.srs, g2)
        assert str(e_new.value) == str(e_old.value)
    # the recovery's table comes first, then the verifier's; a good call follows
    assert retrieve(k, w, rows, bad_value, pf_be, g2, l, bound=count * l + 1)[0] == L.ERR_INVALID_ARG
    dup = rows.copy(); dup[0, 1] = dup[0, 0]
    assert retrieve(k, w, dup, bad_value, pf_be, g2, l)[0] == L.ERR_INVALID_ARG
    rc, ok, _, flags, _, _ = retrieve(k, w, rows, ys_be, pf_be, g2, l)
    assert (rc, ok) == (0, 1) and flags.all()


def test_retrieve_of_one_blob_is_the_single_recovery_through_the_codec(k, world):
    w = world
    L = k._lib
    l = 16
    rows, ys_be, pf_be, g2 = w.chunks(l, seed=2, blobs=1)
    count = rows.shape[1]
    ctx = k.default_context()
    ys, _ = k.verifier.decode_coset_items(ys_be, None, l, ctx=ctx)
    for form in (0, 1):
        out = np.zeros((w.n, 4), dtype=np.uint64)
        flag = C.c_int32(-1)
        assert L.load().kzg_recover_from_cosets(ctx.handle, L.ptr(ys), L.ptr(rows[0].copy()), count, w.n, l, 0, form, L.ptr(out), C.byref(flag)) == 0
        want = k.verifier.encode_coset_items(out.reshape(w.n, 1, 4), None)[0]
        for idx in (rows, rows[0]):
            rc, ok, got, flags, _, _ = retrieve(k, w, idx, ys_be, pf_be, g2, l, form=form, blobs=1)
            assert (rc, ok) == (0, 1) and got == want and flags.tolist() == [flag.value]


# ---- 5. the bound-checked build runs the identity cases above with every site counter at 0 --------------------------------------------------
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
rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", "-x", "tests/test_gpu_recover_bytes.py", "-k",
                  "bit_identity or three_groups or reference_digest"])
counts = (C.c_ulonglong * n)()
first = (C.c_int32 * (9 * n))()
assert h.kzg_bc_read_all(counts, first) == 0
print("PYTEST_RC", int(rc))
for s in range(n):
    print("SITE", s, counts[s])
'''


def test_bound_checked_build_keeps_every_precondition():
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "PYTEST_RC 0" in out, (out[-3000:], res.stderr[-2000:])
    assert " passed" in out and "no tests ran" not in out, out[-1000:]
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert sites
    fired = {int(s[1]): int(s[2]) for s in sites if int(s[2])}
    assert not fired, fired
