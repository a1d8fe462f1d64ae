"""-m gpu: the retriever's call that survives bad chunks (`kzg_retrieve_blobs_bytes_tolerant`) and the located verifier on serialized
items (`kzg_verify_multiproof_batch_locate_bytes`).

Truth.  The status of an item is known from what was planted in it, and for every item that decodes it is checked against
`kzg_verify_multiproof` on the decoded item alone.  The rows and flags of a recovered blob are those of
`kzg_recover_from_cosets_batch_bytes` on the chunks the blob is recovered from (its first use_count good items), and the coefficient rows
are the original blobs.  The located verifier is compared with `kzg_verify_multiproof_batch_locate` on the output of the decode entry.

Shapes.  (16, 1) with 3 blobs; (2048, 16) with 5 blobs of 100 held chunks, 64 used: a blob's segment crosses a 64-lane wave, the second
level's singleton segments sit beside each other; (8192, 2048) with 2 blobs of 3 held chunks, 2 used: the path above 2^10 values per chunk,
where the rejected batch equation has transformed the decoded values in place."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pyref
from coset_bytes_ref import P, x_without_point
from pyref import R_

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
u8p = C.POINTER(C.c_uint8)
i32p = C.POINTER(C.c_int32)
TAU = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/retrieve-tolerant/v1").digest(), "big") % R_
SENTINEL = 0xA5
SHAPES = {
    "tiny": dict(n=16, l=1, B=3, d=8, count=12, use=8),
    "wave": dict(n=2048, l=16, B=5, d=1024, count=100, use=64),
    "long": dict(n=8192, l=2048, B=2, d=4096, count=3, use=2),
}
GOOD, EQUATION, PROOF_BYTES, PROOF_OFF_CURVE, VALUE = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


def be(ints):
    return b"".join(int(v).to_bytes(32, "big") for v in ints)


class World:
    """B polynomials of d coefficients on a known-tau SRS; per blob `count` of the m cosets, chosen and ordered at random, as bytes."""

    def __init__(self, k, name):
        s = SHAPES[name]
        self.k, self.name = k, name
        self.n, self.l, self.B, self.d, self.count, self.use = s["n"], s["l"], s["B"], s["d"], s["count"], s["use"]
        self.m = self.n // self.l
        self.N = self.B * self.count
        self.srs = k.SRS.generate(TAU, self.n)
        self.kz = k.KZG.new()
        rnd = random.Random("retrieve-tolerant/" + name)
        self.coeffs = [[rnd.randrange(R_) for _ in range(self.d)] for _ in range(self.B)]
        polys = [k.PolynomialCoeffForm(pyref.frs_to_mont(c)) for c in self.coeffs]
        self.commitments = np.stack([self.kz.commit_coeff_form(p, self.srs) for p in polys])
        self.commitments_be = k.helpers.compress_g1_be(self.commitments)
        ys, proofs = self.kz.encode_cosets_batch(polys, self.srs, self.n, self.l)
        self.g2 = k.helpers.g2_mul_generator(k.fr.fr_from_int(pow(TAU, self.l, R_)))
        self.rows = np.array([rnd.sample(range(self.m), self.count) for _ in range(self.B)], dtype=np.uint64)
        pick = self.rows.astype(np.int64)
        sel_y = np.ascontiguousarray(np.stack([ys[b][pick[b]] for b in range(self.B)])).reshape(-1, self.l, 4)
        sel_p = np.ascontiguousarray(np.stack([proofs[b][pick[b]] for b in range(self.B)])).reshape(-1, 8)
        self.ys_be, self.pf_be = k.verifier.encode_coset_items(sel_y, sel_p)
        self.original = [be(c) for c in self.coeffs]
        self.ci = [b for b in range(self.B) for _ in range(self.count)]
        self.ki = [int(v) for v in self.rows.reshape(-1)]
        self._truth = {}


_worlds = {}


def world_of(k, name):
    if name not in _worlds:
        _worlds[name] = World(k, name)
    return _worlds[name]


# ---- corruptions: (item, kind) -> bytes and the status the plant implies ---------------------------------------------------------------
def plant(w, plants):
    """Returns (ys_be, pf_be, status (N,) uint8).  Kinds: flip (a value byte), swap (the proof of the NEXT item of the blob, a valid point),
    moved (the whole chunk of the same position of the next blob), x_ge_p, flags00, off_curve, value_r, both (flags00 and a value = r)."""
    ys, pf = bytearray(w.ys_be), bytearray(w.pf_be)
    status = np.zeros(w.N, dtype=np.uint8)
    l, count = w.l, w.count
    for item, kind in plants:
        b, j = divmod(item, count)
        if kind == "flip":
            ys[32 * (item * l + (l - 1)) + 31] ^= 1
            status[item] = EQUATION
        elif kind == "swap":
            other = b * count + (j + 1) % count
            pf[32 * item:32 * item + 32] = w.pf_be[32 * other:32 * other + 32]
            status[item] = EQUATION
        elif kind == "moved":
            other = ((b + 1) % w.B) * count + j
            ys[32 * item * l:32 * (item + 1) * l] = w.ys_be[32 * other * l:32 * (other + 1) * l]
            pf[32 * item:32 * item + 32] = w.pf_be[32 * other:32 * other + 32]
            status[item] = EQUATION
        elif kind == "x_ge_p":
            raw = bytearray(P.to_bytes(32, "big"))
            raw[0] |= 0x80
            pf[32 * item:32 * item + 32] = raw
            status[item] = PROOF_BYTES
        elif kind in ("flags00", "both"):
            pf[32 * item] &= 0x3F
            status[item] = PROOF_BYTES
            if kind == "both":
                ys[32 * item * l:32 * item * l + 32] = R_.to_bytes(32, "big")
        elif kind == "off_curve":
            raw = bytearray(x_without_point(1000 + item).to_bytes(32, "big"))
            raw[0] |= 0x80
            pf[32 * item:32 * item + 32] = raw
            status[item] = PROOF_OFF_CURVE
        elif kind == "value_r":
            at = item * l + (l // 2)
            ys[32 * at:32 * at + 32] = R_.to_bytes(32, "big")
            status[item] = VALUE
        else:
            raise AssertionError(kind)
    return bytes(ys), bytes(pf), status


PLANTS = {
    # blob 0: the first item; blob 1: five bad items, 7 = use_count - 1 good ones left; blob 2: four bad items (the call's last among them), exactly use_count left
    "tiny": [(0, "flip"), (12 + 3, "x_ge_p"), (12 + 4, "value_r"), (12 + 5, "both"), (12 + 6, "off_curve"), (12 + 7, "flip"),
             (24 + 0, "moved"), (24 + 1, "flags00"), (24 + 2, "value_r"), (35, "swap")],
    # blob 0: the first item and the 63rd / 64th sorted item; blob 2: the same places of its own segment; blob 4: a moved chunk and the call's last item; blobs 1 and 3 clean
    "wave": [(0, "flip"), (63, "off_curve"), (64, "swap"), (200 + 63, "value_r"), (200 + 64, "flip"), (200 + 65, "both"), (200 + 99, "swap"),
             (400 + 10, "moved"), (499, "x_ge_p")],
    # blob 0 is recovered from items 0 and 2; blob 1 keeps one good item of three.  (No swapped proof here: with d = 2 l coefficients the quotient
    # of every coset is the blob's upper half, so all proofs of a blob are one point and a swap changes nothing.)
    "long": [(1, "flip"), (3, "value_r"), (5, "moved")],
}


def expected_choice(w, status, use):
    chosen, blob_ok = [], []
    for b in range(w.B):
        good = [j for j in range(w.count) if status[b * w.count + j] == GOOD]
        blob_ok.append(len(good) >= use)
        chosen.append(good[:use])
    return chosen, blob_ok


def reference_rows(w, ys_be, chosen, blob_ok, use, bound, form, out_len):
    """kzg_recover_from_cosets_batch_bytes on the chosen chunks of the recovered blobs; zero rows and flag 0 for the others."""
    rows = out_len or w.n
    want, flags = [bytes(rows * 32)] * w.B, [False] * w.B
    rec = [b for b in range(w.B) if blob_ok[b]]
    if rec:
        idx = np.array([[int(w.rows[b][j]) for j in chosen[b]] for b in rec], dtype=np.uint64)
        picked = b"".join(ys_be[32 * w.l * (b * w.count + j):32 * w.l * (b * w.count + j + 1)] for b in rec for j in chosen[b])
        out, consistent = w.kz.recover_from_cosets_batch_bytes(idx, picked, w.n, w.l, degree_bound=bound or None, eval_form=bool(form), out_len=out_len or None)
        for i, b in enumerate(rec):
            want[b] = out[i * rows * 32:(i + 1) * rows * 32]
            flags[b] = bool(consistent[i])
    return b"".join(want), flags


def tolerant(k, w, ys_be, pf_be, use=None, bound=0, form=0, out_len=0, r_powers=None, commitments_be=None, rows=None):
    """The C entry itself, every output starting from a sentinel: (rc, item status, blob status, bad items, unrecovered, checks, bytes, flags, bad index, bad array)."""
    L = k._lib
    cm = np.frombuffer(commitments_be or w.commitments_be, np.uint8)
    yb, pb = np.frombuffer(ys_be, np.uint8), np.frombuffer(pf_be, np.uint8)
    idx = np.ascontiguousarray(w.rows if rows is None else rows, dtype=np.uint64)
    out = np.full(w.B * (out_len or w.n) * 32, SENTINEL, dtype=np.uint8)
    fl = np.full(w.B, -1, dtype=np.int32)
    ist, bst = np.full(w.N, SENTINEL, dtype=np.uint8), np.full(w.B, SENTINEL, dtype=np.uint8)
    bad_items, unrec, checks = L.sz(1 << 40), L.sz(1 << 40), L.sz(1 << 40)
    bad, arr = C.c_uint64(1 << 40), C.c_int32(-1)
    used = np.full((w.N, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)                        # the weights used: the sentinel of a uint64 array
    rp = None if r_powers is None else np.ascontiguousarray(r_powers, dtype=np.uint64)
    rc = L.load().kzg_retrieve_blobs_bytes_tolerant(L.default_context().handle, w.srs.handle, cm.ctypes.data_as(u8p), L.ptr(idx), 1 if idx.ndim == 1 else w.B,
                                                    yb.ctypes.data_as(u8p), pb.ctypes.data_as(u8p), w.B, w.count, w.use if use is None else use, w.n, w.l, bound, form,
                                                    out_len, None if rp is None else L.ptr(rp), L.ptr(np.ascontiguousarray(w.g2, dtype=np.uint64)),
                                                    ist.ctypes.data_as(u8p), bst.ctypes.data_as(u8p), C.byref(bad_items), C.byref(unrec), C.byref(checks),
                                                    out.ctypes.data_as(u8p), fl.ctypes.data_as(i32p), L.ptr(used), C.byref(bad), C.byref(arr))
    return rc, ist, bst, bad_items.value, unrec.value, checks.value, out.tobytes(), fl, bad.value, arr.value, used


def log2_ceil(v):
    return max(0, (max(v, 1) - 1).bit_length())


def max_checks(groups, bad):
    return 1 + 2 * bad * log2_ceil(groups)


def check_bound(w, status, checks):
    bad_blobs = sum(1 for b in range(w.B) if (status[b * w.count:(b + 1) * w.count] == EQUATION).any())
    bad_items = int((status == EQUATION).sum())
    if bad_items == 0:
        assert checks == 1
    else:
        assert 1 < checks <= 1 + max_checks(w.B, bad_blobs) + max_checks(bad_blobs * w.count, bad_items), (checks, bad_blobs, bad_items)


def planted(k, name):
    """The shape's planted case, run once and shared: (world, ys_be, pf_be, status, result of the entry with coefficient rows cut to d)."""
    w = world_of(k, name)
    if "planted" not in w._truth:
        ys_be, pf_be, status = plant(w, PLANTS[name])
        w._truth["planted"] = (ys_be, pf_be, status, tolerant(k, w, ys_be, pf_be, bound=w.d, form=0, out_len=w.d))
    return (w,) + w._truth["planted"]


# ---- 1. statuses, rows, flags, the bound on the pairing checks -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_bad_chunks_are_named_and_the_blobs_recovered_from_the_good_ones(k, name):
    w, ys_be, pf_be, status, res = planted(k, name)
    rc, ist, bst, n_bad, n_unrec, checks, got, flags = res[:8]
    print(name, "pairing checks", checks, "bad items", n_bad, "unrecovered", n_unrec)
    assert rc == 0
    assert np.array_equal(ist, status), (ist.reshape(w.B, -1), status.reshape(w.B, -1))
    chosen, blob_ok = expected_choice(w, status, w.use)
    assert bst.tolist() == [0 if ok else 1 for ok in blob_ok]
    assert (n_bad, n_unrec) == (int((status != 0).sum()), blob_ok.count(False))
    check_bound(w, status, checks)
    want, want_flags = reference_rows(w, ys_be, chosen, blob_ok, w.use, w.d, 0, w.d)
    assert got == want and flags.tolist() == [1 if f else 0 for f in want_flags]
    for b in range(w.B):                                                                # the coefficient rows are the original blobs, or zero
        row = got[b * w.d * 32:(b + 1) * w.d * 32]
        assert row == (w.original[b] if blob_ok[b] else bytes(w.d * 32)) and flags[b] == (1 if blob_ok[b] else 0)
    if name == "tiny":
        assert blob_ok == [True, False, True] and len([s for s in status[24:36] if s == GOOD]) == w.use    # use_count - 1 good items: not recovered; exactly use_count: recovered
    # evaluation rows, the default form of the Python surface
    ist2, ok2, polys2, cons2 = k.verifier.retrieve_blobs_bytes_tolerant(w.commitments_be, w.rows, ys_be, pf_be, w.n, w.l, w.srs, use_count=w.use, g2_tau_l=w.g2)
    want2, want_flags2 = reference_rows(w, ys_be, chosen, blob_ok, w.use, 0, 1, 0)
    assert np.array_equal(ist2.reshape(-1), status) and ok2.tolist() == blob_ok and polys2 == want2 and cons2.tolist() == want_flags2


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_status_of_every_decodable_item_is_that_of_the_single_verifier(k, name):
    w, ys_be, pf_be, status, res = planted(k, name)
    ist = res[1]
    touched = {item // w.count for item, _ in PLANTS[name]}
    items = [i for i in range(w.N) if status[i] in (GOOD, EQUATION) and (i // w.count in touched or i % w.count in (0, w.count - 1))]
    sel_y = b"".join(ys_be[32 * w.l * i:32 * w.l * (i + 1)] for i in items)
    sel_p = b"".join(pf_be[32 * i:32 * i + 32] for i in items)
    ys, pf = k.verifier.decode_coset_items(sel_y, sel_p, w.l)
    for at, i in enumerate(items):
        ok = k.verifier.verify_multiproof(w.commitments[i // w.count], pf[at], w.ki[i], ys[at], w.n, w.srs, w.g2)
        assert ok == (status[i] == GOOD) and ist[i] == (GOOD if ok else EQUATION), i
    for i in range(w.N):                                                                # the refused ones do not decode, for the reason reported
        if status[i] in (PROOF_BYTES, PROOF_OFF_CURVE):
            with pytest.raises(k.errors.NotOnCurveError if status[i] == PROOF_OFF_CURVE else k.errors.DeserializationError, match="proof 0"):
                k.verifier.decode_coset_items(None, pf_be[32 * i:32 * i + 32], w.l)
        if status[i] == VALUE:
            with pytest.raises(k.errors.DeserializationError, match="value of item 0"):
                k.verifier.decode_coset_items(ys_be[32 * w.l * i:32 * w.l * (i + 1)], None, w.l)


# ---- 2. nothing bad ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_nothing_bad_and_every_chunk_used_is_the_all_or_nothing_call(k, name):
    w = world_of(k, name)
    for form in (0, 1):
        rc, ist, bst, n_bad, n_unrec, checks, got, flags, _, _, _ = tolerant(k, w, w.ys_be, w.pf_be, use=w.count, form=form)
        ok, polys, consistent = k.verifier.retrieve_blobs_bytes(w.commitments_be, w.rows, w.ys_be, w.pf_be, w.n, w.l, w.srs, w.g2, eval_form=bool(form))
        assert ok is True and rc == 0 and got == polys and flags.tolist() == [int(c) for c in consistent]
        assert not ist.any() and not bst.any() and (n_bad, n_unrec, checks) == (0, 0, 1)
    # fewer chunks used than held: still one check, the rows are the blobs
    rc, ist, bst, _, _, checks, got, flags, _, _, _ = tolerant(k, w, w.ys_be, w.pf_be, bound=w.d, out_len=w.d)
    assert rc == 0 and checks == 1 and got == b"".join(w.original) and flags.all() and not ist.any() and not bst.any()
    # a degree bound below the true degree: the good chunks verify, the flag says the degree is not below the bound
    rc, _, bst, _, _, _, got, flags, _, _, _ = tolerant(k, w, w.ys_be, w.pf_be, bound=w.d - 1, out_len=w.d)
    assert rc == 0 and got == b"".join(w.original) and flags.tolist() == [0] * w.B and not bst.any()


def test_one_index_row_for_all_blobs(k):
    w = world_of(k, "tiny")
    kz, polys = w.kz, [k.PolynomialCoeffForm(pyref.frs_to_mont(c)) for c in w.coeffs]
    ys, proofs = kz.encode_cosets_batch(polys, w.srs, w.n, w.l)
    row = w.rows[1].astype(np.int64)
    sel_y = np.ascontiguousarray(np.stack([ys[b][row] for b in range(w.B)])).reshape(-1, w.l, 4)
    sel_p = np.ascontiguousarray(np.stack([proofs[b][row] for b in range(w.B)])).reshape(-1, 8)
    ys_be, pf_be = k.verifier.encode_coset_items(sel_y, sel_p)
    rc, ist, bst, _, _, checks, got, flags, _, _, _ = tolerant(k, w, ys_be, pf_be, bound=w.d, out_len=w.d, rows=w.rows[1])
    assert rc == 0 and checks == 1 and got == b"".join(w.original) and flags.all() and not ist.any()
    bad = bytearray(ys_be)
    bad[32 * (w.count + 2) + 31] ^= 1                                                   # item 2 of blob 1: the blobs' choices now differ
    rc, ist, bst, n_bad, _, checks, got, flags, _, _, _ = tolerant(k, w, bytes(bad), pf_be, bound=w.d, out_len=w.d, rows=w.rows[1])
    want = np.zeros(w.N, np.uint8)
    want[w.count + 2] = EQUATION
    assert rc == 0 and np.array_equal(ist, want) and n_bad == 1 and got == b"".join(w.original) and flags.all() and not bst.any()


# ---- 3. every blob bad -----------------------------------------------------------------------------------------------------------------------
def test_every_blob_bad(k):
    w = world_of(k, "tiny")
    kinds = ("flip", "x_ge_p", "value_r", "off_curve", "swap", "flags00")
    plants = [(b * w.count + j, kinds[(b + j) % len(kinds)]) for b in range(w.B) for j in range(w.count - w.use + 1)]     # use_count - 1 good items everywhere
    ys_be, pf_be, status = plant(w, plants)
    rc, ist, bst, n_bad, n_unrec, checks, got, flags, _, _, _ = tolerant(k, w, ys_be, pf_be, bound=w.d, out_len=w.d)
    assert rc == 0 and np.array_equal(ist, status) and bst.tolist() == [1] * w.B and n_unrec == w.B and n_bad == len(plants)
    assert got == bytes(w.B * w.d * 32) and flags.tolist() == [0] * w.B
    check_bound(w, status, checks)
    everything = [(i, kinds[i % len(kinds)]) for i in range(w.N)]                        # not one good item in the call
    ys_be, pf_be, status = plant(w, everything)
    rc, ist, bst, n_bad, n_unrec, checks, got, flags, _, _, _ = tolerant(k, w, ys_be, pf_be)
    assert rc == 0 and np.array_equal(ist, status) and n_bad == w.N and n_unrec == w.B and got == bytes(w.B * w.n * 32) and not flags.any()
    check_bound(w, status, checks)


# ---- 4. weights: supplied, derived on the host, derived on the device -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "wave"])
def test_supplied_and_derived_weights_give_the_same_answer(k, name):
    w, ys_be, pf_be, status, res = planted(k, name)
    ctx = k.default_context()
    weights = k.verifier.compute_multiproof_r_powers_bytes(w.commitments_be, w.ci, w.ki, ys_be, pf_be, w.n, w.l)    # the bytes as given, refusals included
    try:
        for mode, rp in ((0, weights), (1, None), (2, None)):
            ctx.set_transcript_device(mode)
            got = tolerant(k, w, ys_be, pf_be, bound=w.d, form=0, out_len=w.d, r_powers=rp)
            assert got[0] == 0 and np.array_equal(got[1], status) and np.array_equal(got[2], res[2]) and got[3:5] == res[3:5], mode
            assert got[6] == res[6] and np.array_equal(got[7], res[7]), mode
            check_bound(w, status, got[5])
            # the weights used, on every path: the bits of the bytes transcript on the bytes AS GIVEN -- refused chunks hashed as they came --
            # at every item that decodes, zero at every refused one
            refused = status >= PROOF_BYTES
            assert refused.any() and np.array_equal(got[10][~refused], weights[~refused]) and not got[10][refused].any(), mode
            assert weights[refused].any(axis=1).all()                                   # (the transcript's own weights there are not zero)
    finally:
        ctx.set_transcript_device(0)


# ---- 5. several recovery groups ---------------------------------------------------------------------------------------------------------------
def test_several_recovery_groups(k):
    w, ys_be, pf_be, status, res = planted(k, "wave")
    ctx = k.default_context()
    per = k.helpers.recover_batch_info(w.B, w.use, w.n, w.l)["blob_bytes"]
    assert k.helpers.recover_batch_info(w.B, w.use, w.n, w.l, 0, 2 * per)["groups"] == 3
    try:
        ctx.set_recover_group_bytes(2 * per)
        got = tolerant(k, w, ys_be, pf_be, bound=w.d, form=0, out_len=w.d)
        clean = tolerant(k, w, w.ys_be, w.pf_be, form=1)
    finally:
        ctx.set_recover_group_bytes(0)
    assert got[0] == 0 and np.array_equal(got[1], status) and got[6] == res[6] and np.array_equal(got[7], res[7])
    assert clean[0] == 0 and clean[6] == tolerant(k, w, w.ys_be, w.pf_be, form=1)[6]


# ---- 6. errors: the outputs stay at the sentinel ----------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_alone(k):
    L = k._lib
    w = world_of(k, "tiny")

    def untouched(r):
        return (set(r[1]) == {SENTINEL} and set(r[2]) == {SENTINEL} and set(r[6]) == {SENTINEL} and (r[7] == -1).all() and r[3] == r[4] == r[5] == 1 << 40
                and (r[10] == 0xA5A5A5A5A5A5A5A5).all())
    for kwargs, status in ((dict(use=0), L.ERR_INVALID_ARG), (dict(use=w.count + 1), L.ERR_INVALID_ARG), (dict(bound=w.use * w.l + 1), L.ERR_INVALID_ARG),
                           (dict(out_len=w.use * w.l - 1), L.ERR_INVALID_ARG), (dict(form=1, out_len=w.n - 1), L.ERR_INVALID_ARG)):
        r = tolerant(k, w, w.ys_be, w.pf_be, **kwargs)
        assert r[0] == status and untouched(r), kwargs
    dup = w.rows.copy()
    dup[2, w.count - 1] = dup[2, 0]                                                     # a held item beyond the first use_count
    assert tolerant(k, w, w.ys_be, w.pf_be, rows=dup)[0] == L.ERR_INVALID_ARG
    # a commitment that does not decode is the retriever's own input: a call error, as in the all-or-nothing entry
    bad_cm = bytearray(w.commitments_be)
    bad_cm[32:64] = P.to_bytes(32, "big")
    bad_cm[32] |= 0x80
    ys_be, pf_be, _ = plant(w, [(0, "value_r"), (5, "flags00")])                        # refused items beside it do not take its place
    r = tolerant(k, w, ys_be, pf_be, commitments_be=bytes(bad_cm))
    assert (r[0], r[8], r[9]) == (L.ERR_DESERIALIZE, 1, 0) and untouched(r)
    with pytest.raises(k.errors.DeserializationError, match="commitment 1"):
        k.verifier.retrieve_blobs_bytes_tolerant(bytes(bad_cm), w.rows, ys_be, pf_be, w.n, w.l, w.srs, use_count=w.use, g2_tau_l=w.g2)
    g2_bad = np.array(w.g2, dtype=np.uint64).copy()
    g2_bad[0] ^= 1
    saved, w.g2 = w.g2, g2_bad                                                          # behind the refused items, which end no call
    try:
        r = tolerant(k, w, ys_be, pf_be)
    finally:
        w.g2 = saved
    assert r[0] == L.ERR_G2_TAU_NOT_ON_CURVE and untouched(r)
    r = tolerant(k, w, w.ys_be, w.pf_be, bound=w.d, out_len=w.d)                        # the context is as usable as before
    assert r[0] == 0 and r[6] == b"".join(w.original)


# ---- 7. kzg_verify_multiproof_batch_locate_bytes against the decoded entry ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_locate_bytes_is_the_decoded_entry(k, name):
    w = world_of(k, name)
    v = k.verifier
    plants = [(i, kind) for i, kind in PLANTS[name] if kind in ("flip", "swap", "moved")]     # what decodes
    ys_be, pf_be, status = plant(w, plants)
    ys, pf = v.decode_coset_items(ys_be, pf_be, w.l)
    rnd = random.Random(name)
    partition = [rnd.randrange(7) for _ in range(w.N)]
    for groups, n_groups in (("commitment", None), ("item", None), (partition, 9)):
        want, want_checks = v.locate_bad_multiproofs(w.commitments, w.ci, w.ki, ys, pf, w.n, w.srs, w.g2, groups=groups, n_groups=n_groups)
        good, checks, used = v.locate_bad_multiproofs_bytes(w.commitments_be, w.ci, w.ki, ys_be, pf_be, w.n, w.l, w.srs, w.g2, groups=groups, n_groups=n_groups,
                                                            return_r_powers=True)
        assert np.array_equal(good, want) and checks == want_checks, groups if isinstance(groups, str) else "partition"
        assert np.array_equal(used, v.compute_multiproof_r_powers(w.commitments, w.ci, w.ki, ys, pf, w.n))           # bit for bit
        assert np.array_equal(used, v.compute_multiproof_r_powers_bytes(w.commitments_be, w.ci, w.ki, ys_be, pf_be, w.n, w.l))
        if groups == "item":
            assert np.array_equal(~good, status == EQUATION)
        if groups == "commitment":
            assert (~good).tolist() == [bool((status[b * w.count:(b + 1) * w.count] == EQUATION).any()) for b in range(w.B)]
    weights = v.compute_multiproof_r_powers_bytes(w.commitments_be, w.ci, w.ki, ys_be, pf_be, w.n, w.l)
    ctx = k.default_context()
    try:
        for mode, rp in ((0, weights), (1, None), (2, None)):                           # supplied, host transcript, device transcript
            ctx.set_transcript_device(mode)
            good, checks, used = v.locate_bad_multiproofs_bytes(w.commitments_be, w.ci, w.ki, ys_be, pf_be, w.n, w.l, w.srs, w.g2, r_powers=rp, groups="item",
                                                                return_r_powers=True)
            assert np.array_equal(~good, status == EQUATION) and np.array_equal(used, weights), mode
    finally:
        ctx.set_transcript_device(0)
    good, checks = v.locate_bad_multiproofs_bytes(w.commitments_be, w.ci, w.ki, w.ys_be, w.pf_be, w.n, w.l, w.srs, w.g2)
    assert good.all() and checks == 1                                                   # a good batch: the root alone


def test_locate_bytes_refuses_as_the_batch_entry_on_bytes(k):
    L = k._lib
    v = k.verifier
    w = world_of(k, "tiny")
    bad_cm = bytearray(w.commitments_be)
    bad_cm[64:96] = P.to_bytes(32, "big")
    bad_cm[64] |= 0x80
    cases = [plant(w, [(7, "value_r"), (20, "value_r")])[:2] + (w.commitments_be,), plant(w, [(9, "flags00"), (4, "off_curve"), (2, "value_r")])[:2] + (w.commitments_be,),
             plant(w, [(30, "x_ge_p")])[:2] + (w.commitments_be,), plant(w, [(1, "flags00")])[:2] + (bytes(bad_cm),)]
    for ys_be, pf_be, cm in cases:
        with pytest.raises((k.errors.DeserializationError, k.errors.NotOnCurveError)) as e_old:
            v.verify_multiproof_batch_bytes(cm, w.ci, w.ki, ys_be, pf_be, w.n, w.l, w.srs, w.g2)
        with pytest.raises((k.errors.DeserializationError, k.errors.NotOnCurveError)) as e_new:
            v.locate_bad_multiproofs_bytes(cm, w.ci, w.ki, ys_be, pf_be, w.n, w.l, w.srs, w.g2, groups="item")
        assert type(e_new.value) is type(e_old.value) and str(e_new.value) == str(e_old.value)
    # the grouped host checks come first: a group index = n_groups in front of bytes that do not decode
    ys_be, pf_be, _ = plant(w, [(0, "value_r")])
    with pytest.raises(ValueError, match="invalid argument"):
        v.locate_bad_multiproofs_bytes(w.commitments_be, w.ci, w.ki, ys_be, pf_be, w.n, w.l, w.srs, w.g2, groups=[3] * w.N, n_groups=3)
    # ... and the order of the grouped host checks, each in front of everything behind it, all in front of the bytes: a null pointer, the G2
    # point that chunks of more than one value need, the SRS, n, the chunk length, the SRS's capacity, a coset index, a commitment row, a group index
    lib, ctx_h = L.load(), L.default_context().handle
    cm_a, ys_a, pf_a = (np.frombuffer(x, np.uint8) for x in (w.commitments_be, ys_be, pf_be))
    ci_a, ki_a, g2_a = np.array(w.ci, np.uint64), np.array(w.ki, np.uint64), np.ascontiguousarray(w.g2, dtype=np.uint64)
    ok_a, nb_a = np.zeros(w.N, np.uint8), L.sz(0)

    def raw(ys=ys_a, ki=ki_a, ci=ci_a, n=w.n, l=w.l, gi=None, n_groups=w.N, srs=w.srs.handle, out_bad=C.byref(nb_a), count=w.N, g2=g2_a):
        gi = np.arange(w.N, dtype=np.uint64) if gi is None else gi
        return lib.kzg_verify_multiproof_batch_locate_bytes(ctx_h, srs, cm_a.ctypes.data_as(u8p), w.B, L.ptr(ci), L.ptr(ki), None if ys is None else ys.ctypes.data_as(u8p),
                                                            pf_a.ctypes.data_as(u8p), count, n, l, None, None if g2 is None else L.ptr(g2), L.ptr(gi), n_groups,
                                                            ok_a.ctypes.data_as(u8p), out_bad, None, None, None, None)
    bad_gi, bad_ki, bad_ci = np.full(w.N, w.N, np.uint64), ki_a.copy(), ci_a.copy()
    bad_ki[3], bad_ci[5] = 1 << 40, w.B
    assert raw(out_bad=None, n=96) == L.ERR_INVALID_ARG and raw(ys=None, n=96) == L.ERR_INVALID_ARG            # null pointers in front of the shape
    assert raw(g2=None, l=4, n=96) == L.ERR_INVALID_ARG and raw(srs=None, n=96) == L.ERR_INVALID_ARG
    assert raw(n=96, l=3) == L.ERR_NOT_POWER_OF_TWO and raw(n=1 << 25, l=3) == L.ERR_DOMAIN                      # n in front of the chunk length
    assert raw(l=3, ki=bad_ki) == L.ERR_INVALID_ARG
    assert raw(n=1 << 16, l=1 << 5, ki=bad_ki) == L.ERR_SRS_CAPACITY_EXCEEDED                                    # the SRS (16 points) in front of the indices
    assert raw(ki=bad_ki, gi=bad_gi) == L.ERR_INVALID_ARG and raw(ci=bad_ci, gi=bad_gi) == L.ERR_INVALID_ARG
    assert raw(gi=bad_gi) == L.ERR_INVALID_ARG and raw() == L.ERR_DESERIALIZE                                     # the group index in front of the bytes
    # count = 0: every group good, no device work, no pairing check; the outputs start from a sentinel
    good = np.full(4, SENTINEL, np.uint8)
    n_bad, checks = L.sz(1 << 40), L.sz(1 << 40)
    cm = np.frombuffer(w.commitments_be, np.uint8)
    rc = L.load().kzg_verify_multiproof_batch_locate_bytes(L.default_context().handle, w.srs.handle, cm.ctypes.data_as(u8p), w.B, None, None, None, None, 0, w.n, w.l, None,
                                                           L.ptr(np.ascontiguousarray(w.g2, dtype=np.uint64)), None, 4, good.ctypes.data_as(u8p), C.byref(n_bad),
                                                           C.byref(checks), None, None, None)
    assert rc == 0 and good.tolist() == [1, 1, 1, 1] and (n_bad.value, checks.value) == (0, 0)


# ---- 8. the bound-checked build runs one case per shape with every site counter at 0 ------------------------------------------------------------
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
rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", "-x", "tests/test_gpu_retrieve_tolerant.py", "-k", "bad_chunks_are_named or locate_bytes_is_the_decoded"])
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
