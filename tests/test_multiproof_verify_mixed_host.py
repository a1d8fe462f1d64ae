"""CPU-only checks of the verification of coset proofs of MIXED shapes (`kzg_verify_multiproof_batch_mixed`): the mixed equation restated
over Fr with a known tau, the transcript of `kzg_compute_multiproof_r_powers_mixed` (host-only C) against hashlib, the declarations of the
three entries, the argument errors that need no device, and the host check program (planner, permutation, scalars, error order) as a
plain g++ executable and again under ASan + UBSan."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import coset_mixed_ref
import coset_ref
import pyref
from pyref import R_, dft, poly_eval, root_of_unity

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
ENTRIES = ("kzg_coset_interpolate_rlc_mixed", "kzg_compute_multiproof_r_powers_mixed", "kzg_verify_multiproof_batch_mixed")


def quotient_at(f, l, c, tau):
    """[f / (X^l - c)](tau), the remainder dropped"""
    f = list(f)
    q = [0] * (len(f) - l)
    for i in range(len(f) - 1, l - 1, -1):
        q[i - l] = f[i]
        f[i - l] = (f[i - l] + f[i] * c) % R_
    return poly_eval(q, tau)


# ---- the equation ---------------------------------------------------------------------------------------------------------------------
CLASSES = [(64, 4), (32, 4), (64, 1), (256, 16), (16, 8)]            # two classes of equal l and different n; an empty class (16, 8)


def _world(seed):
    """One polynomial per class that has items (its degree below the class's n), 14 items over the classes in shuffled order with a repeat."""
    rnd = random.Random(seed)
    tau = rnd.randrange(2, R_)
    polys, evals, commitments = [], [], []
    for n, _ in CLASSES[:4]:
        f = [rnd.randrange(R_) for _ in range(n)]
        polys.append(f)
        evals.append(dft(f))
        commitments.append(poly_eval(f, tau))
    class_indices = [0, 1, 2, 3, 0, 1, 2, 3, 1, 1, 0, 3, 2, 0]
    rnd.shuffle(class_indices)
    rows = list(class_indices)                                        # commitment row = the class's polynomial
    ks = [rnd.randrange(CLASSES[s][0] // CLASSES[s][1]) for s in class_indices]
    j = [i for i, s in enumerate(class_indices) if s == 1]
    ks[j[1]] = ks[j[0]]                                               # the same item twice
    ks[[i for i, s in enumerate(class_indices) if s == 0][0]] = CLASSES[0][0] // CLASSES[0][1] - 1     # k = m - 1: >= the m of class 1
    ys, proofs = [], []
    for s, k in zip(class_indices, ks):
        n, l = CLASSES[s]
        ys.append(evals[s][k::n // l])
        proofs.append(quotient_at(polys[s], l, pow(root_of_unity(n.bit_length() - 1), k * l, R_), tau))
    r = rnd.randrange(R_)
    weights = [pow(r, i, R_) for i in range(len(ks))]
    return tau, commitments, class_indices, rows, ks, ys, proofs, weights


@pytest.mark.parametrize("seed", [1, 2])
def test_mixed_equation_over_fr_with_a_known_tau(seed):
    """tau known, group elements as discrete logarithms.  Four classes with items, (64, 4) and (32, 4) sharing one G2 pair, in shuffled
    order: the equation holds, and fails when one value, one proof, one coset index or one class index is changed.  Moving an item
    between the two l = 4 classes changes only w_s (same pair, same value count), which is what the fault pins."""
    tau, commitments, si, rows, ks, ys, proofs, weights = _world(seed)
    holds = lambda **kw: coset_mixed_ref.mixed_equation_holds(tau, CLASSES, kw.get("si", si), commitments, rows, kw.get("ks", ks),   # noqa: E731
                                                              kw.get("ys", ys), kw.get("proofs", proofs), weights, kw.get("tau_powers"))
    assert holds()
    # every item alone, weight 1
    for i in range(len(ks)):
        assert coset_mixed_ref.mixed_equation_holds(tau, CLASSES, [si[i]], commitments, [rows[i]], [ks[i]], [ys[i]], [proofs[i]], [1])
    # one class only: the uniform equation
    sel = [i for i, s in enumerate(si) if s == 3]
    assert coset_ref.batch_equation_holds(tau, 256, 16, commitments, [rows[i] for i in sel], [ks[i] for i in sel], [ys[i] for i in sel],
                                          [proofs[i] for i in sel], [weights[i] for i in sel])
    for s in range(4):
        i = si.index(s)
        bad = [list(y) for y in ys]
        bad[i][-1] = (bad[i][-1] + 1) % R_
        assert not holds(ys=bad), s
        badp = list(proofs)
        badp[i] = (badp[i] + 1) % R_
        assert not holds(proofs=badp), s
        badk = list(ks)
        badk[i] = (badk[i] + 1) % (CLASSES[s][0] // CLASSES[s][1])
        assert not holds(ks=badk), s
    i = next(i for i, s in enumerate(si) if s == 1 and ks[i] != 0)    # (32, 4) -> (64, 4): same l, k < 8 is valid in both
    moved = list(si)
    moved[i] = 0
    assert not holds(si=moved)
    # a class's G2 point replaced by [tau^(2 l)]_2
    for s in (0, 2, 3):
        tp = [pow(tau, l, R_) for _, l in CLASSES]
        tp[s] = pow(tau, 2 * CLASSES[s][1], R_)
        assert not holds(tau_powers=tp), s
    # A_t against its definition, column by column
    A = coset_mixed_ref.mixed_rlc(CLASSES, si, ks, ys, weights)
    assert len(A) == 16
    w64, w32 = root_of_unity(6), root_of_unity(5)
    assert pow(w64, 2, R_) == w32                                      # w_s = w_max^(n_max / n_s)
    for t in range(16):
        tot = 0
        for s, k, y, r in zip(si, ks, ys, weights):
            n, l = CLASSES[s]
            if l > t:
                tot += r * pow(root_of_unity(n.bit_length() - 1), -k * t, R_) * coset_ref.ifft(y)[t]
        assert A[t] == tot % R_, t


# ---- the transcript -------------------------------------------------------------------------------------------------------------------
def _random_point(rnd):
    return pyref.ec_mul(rnd.randrange(1, R_), (1, 2))


def _transcript_world(count, seed):
    rnd = random.Random(seed)
    classes = [(64, 4), (32, 4), (64, 1), (256, 16), (16, 8)]
    pool = [_random_point(rnd) for _ in range(4)] + [None]
    commitments = [pool[0], pool[4], pool[1]]
    proofs = [pool[rnd.randrange(5)] for _ in range(count)]
    proofs[0] = None
    si = [rnd.randrange(4) for _ in range(count)]
    if count > 2:
        si[1], si[2] = 0, 1
    rows = [rnd.randrange(3) for _ in range(count)]
    ks = [rnd.randrange(classes[s][0] // classes[s][1]) for s in si]
    ys = [[rnd.randrange(R_) for _ in range(classes[s][1])] for s in si]
    ys[0][0] = 0
    ys[-1][-1] = R_ - 1
    return classes, commitments, proofs, si, rows, ks, ys


def _wire_pt(p):
    return np.zeros(8, np.uint64) if p is None else pyref.point_to_wire(p)


def _c_r_powers(classes, commitments, proofs, si, rows, ks, ys, flat=False):
    from rust_kzg_bn254_amd import verifier
    ys_w = [pyref.frs_to_mont(y) for y in ys]
    if flat:
        ys_w = np.concatenate(ys_w)
    return verifier.compute_multiproof_r_powers_mixed([_wire_pt(c) for c in commitments], rows, classes, si, ks, ys_w, [_wire_pt(p) for p in proofs])


@pytest.mark.parametrize("count", [1, 2, 33, 300])
def test_r_powers_mixed_c_abi_matches_the_hashlib_restatement(count):
    """`kzg_compute_multiproof_r_powers_mixed` bit for bit against coset_mixed_ref.mixed_r: identity points, y = 0 and y = r - 1, ragged
    values given per item and as one flat array.  Moving an item to another class of the same l, swapping two class rows, or changing any
    single input changes r."""
    classes, commitments, proofs, si, rows, ks, ys = _transcript_world(count, 40 + count)
    got = _c_r_powers(classes, commitments, proofs, si, rows, ks, ys)
    r = coset_mixed_ref.mixed_r(classes, si, commitments, rows, ks, ys, proofs)
    assert pyref.frs_from_mont(got) == [pow(r, i, R_) for i in range(count)]
    assert np.array_equal(got, _c_r_powers(classes, commitments, proofs, si, rows, ks, ys, flat=True))
    if count < 3:
        return
    r_of = lambda **kw: pyref.fr_from_mont(_c_r_powers(kw.get("classes", classes), kw.get("commitments", commitments), kw.get("proofs", proofs),   # noqa: E731
                                                       kw.get("si", si), kw.get("rows", rows), kw.get("ks", ks), kw.get("ys", ys))[1])
    seen = {r}
    assert r_of() == r
    moved = list(si)
    moved[2] = 0                                                      # class (32, 4) -> (64, 4): the same values and coset index fit
    swapped_classes = [classes[1], classes[0]] + classes[2:]          # two class rows swapped, the items keep their indices
    ys2 = [list(y) for y in ys]
    ys2[-1][-1] = 5
    rows2 = list(rows); rows2[1] = (rows2[1] + 1) % 3
    ks2 = list(ks); ks2[-1] = (ks2[-1] + 1) % (classes[si[-1]][0] // classes[si[-1]][1])
    proofs2 = list(proofs); proofs2[-1] = commitments[0] if proofs[-1] != commitments[0] else commitments[2]
    commitments2 = [commitments[0], None, _random_point(random.Random(5))]
    other_n = [(128, 4)] + classes[1:]
    for kw in (dict(si=moved), dict(classes=swapped_classes), dict(ys=ys2), dict(rows=rows2), dict(ks=ks2), dict(proofs=proofs2),
               dict(commitments=commitments2), dict(classes=other_n), dict(classes=classes + [(8, 2)])):
        v = r_of(**kw)
        assert v == coset_mixed_ref.mixed_r(kw.get("classes", classes), kw.get("si", si), kw.get("commitments", commitments), kw.get("rows", rows),
                                            kw.get("ks", ks), kw.get("ys", ys), kw.get("proofs", proofs)), kw.keys()
        assert v not in seen, kw.keys()
        seen.add(v)


def test_one_class_transcript_is_not_the_uniform_one():
    """The same items through the uniform and the mixed transcript: different tags, different r (a batch is bound to the entry it was
    derived for)."""
    from rust_kzg_bn254_amd import verifier
    classes, commitments, proofs, si, rows, ks, ys = _transcript_world(5, 9)
    si = [3] * 5
    ks = [k % 16 for k in range(5)]
    ys = [[(7 * i + j) % R_ for j in range(16)] for i in range(5)]
    a = _c_r_powers(classes, commitments, proofs, si, rows, ks, ys)
    b = verifier.compute_multiproof_r_powers([_wire_pt(c) for c in commitments], rows, ks, np.stack([pyref.frs_to_mont(y) for y in ys]),
                                             [_wire_pt(p) for p in proofs], 256)
    assert not np.array_equal(a[1], b[1])


# ---- declarations and the errors that need no device --------------------------------------------------------------------------------------
def test_header_prototypes_and_exports_agree_on_the_three_entries():
    import rust_kzg_bn254_amd as k
    hdr = open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read()
    lib = C.CDLL(k._lib.LIB_PATH)
    for name in ENTRIES:
        assert name in k._lib.PROTOTYPES, name
        assert hasattr(lib, name), name
        decl = re.search(r"\bint32_t %s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(k._lib.PROTOTYPES[name][1]), name
    assert callable(k.verify_multiproof_batch_mixed) and callable(k.verifier.compute_multiproof_r_powers_mixed)
    assert callable(k.helpers.coset_interpolate_rlc_mixed)
    fs = open(os.path.join(CSRC, "host_fiat_shamir.h")).read()
    assert 'COSET_MIXED_DOMAIN[] = "KZGBN254_COSETMIXED__V1_"' in fs and len("KZGBN254_COSETMIXED__V1_") == 24


class _FakeSrs:
    handle = None

    def __len__(self):
        return 64


def test_argument_errors_that_need_no_device():
    """Null handles through the C-ABI (every call returns before it needs a context), the host-only entry's own table, and the Python
    surface's shape checks, which must not create a context."""
    import rust_kzg_bn254_amd as k
    from rust_kzg_bn254_amd import verifier
    lib = k.load()
    L = k._lib
    ok = L.i32(7)
    pt = np.zeros((1, 8), np.uint64)
    idx = np.zeros(1, np.uint64)
    cn, cl = np.array([8], np.uint64), np.array([2], np.uint64)
    ys = np.zeros((2, 4), np.uint64)
    one = pyref.frs_to_mont([1])
    g2 = np.ascontiguousarray(k.helpers.g2_generator()).reshape(1, 16)
    P = L.ptr
    assert lib.kzg_verify_multiproof_batch_mixed(None, None, P(pt), 1, P(idx), P(cn), P(cl), 1, P(idx), P(idx), P(ys), P(pt), 1, P(one), P(g2),
                                                 C.byref(ok)) == L.ERR_INVALID_ARG
    assert lib.kzg_coset_interpolate_rlc_mixed(None, P(cn), P(cl), 1, P(idx), P(idx), P(ys), P(one), 1, P(ys)) == L.ERR_INVALID_ARG
    assert ok.value == 7
    out = np.zeros((1, 4), np.uint64)
    rp = lambda **kw: lib.kzg_compute_multiproof_r_powers_mixed(P(pt), 1, kw.get("ci", P(idx)), kw.get("cn", P(cn)), kw.get("cl", P(cl)), kw.get("S", 1),   # noqa: E731
                                                                kw.get("si", P(idx)), P(idx), P(ys), P(pt), kw.get("count", 1), kw.get("out", P(out)))
    assert rp() == L.OK and out.any()
    one_idx, zero_len, long_len = np.array([1], np.uint64), np.array([0], np.uint64), np.array([(1 << 28) + 1], np.uint64)
    for kw in (dict(ci=None), dict(cn=None), dict(cl=None), dict(si=None), dict(out=None), dict(S=0), dict(si=P(one_idx)), dict(cl=P(zero_len))):
        assert rp(**kw) == L.ERR_INVALID_ARG, kw
    assert rp(cl=P(long_len)) == L.ERR_TOO_LARGE
    assert lib.kzg_compute_multiproof_r_powers_mixed(None, 0, None, None, None, 0, None, None, None, None, 0, None) == L.OK
    before = dict(k._lib._default_ctx)                                          # device id -> Context: must not grow
    with pytest.raises(k.errors.GenericError, match="one point per class"):
        verifier.verify_multiproof_batch_mixed([pt[0]], [0], [(8, 2)], [0], [0], [ys], [pt[0]], _FakeSrs(), [])
    with pytest.raises(k.errors.GenericError, match="not the same"):
        verifier.verify_multiproof_batch_mixed([pt[0]], [0, 0], [(8, 2)], [0], [0], [ys], [pt[0]], _FakeSrs(), g2)
    with pytest.raises(k.errors.InvalidInputLength):                            # a value row of the wrong length
        verifier.verify_multiproof_batch_mixed([pt[0]], [0], [(8, 2)], [0], [0], [np.zeros((3, 4), np.uint64)], [pt[0]], _FakeSrs(), g2)
    with pytest.raises(k.errors.InvalidInputLength):                            # a flat array of the wrong total
        verifier.verify_multiproof_batch_mixed([pt[0]], [0], [(8, 2)], [0], [0], np.zeros((3, 4), np.uint64), [pt[0]], _FakeSrs(), g2)
    assert k._lib._default_ctx == before


# ---- the host check program ------------------------------------------------------------------------------------------------------------
def _build_and_run(tmp, flags):
    exe = str(tmp / "cosetmixedcheck")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", *flags, "-I" + CSRC,
                           os.path.join(HERE, "hostcheck", "cosetmixedcheck.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def test_host_check_program_plain_and_sanitized(tmp_path):
    """tests/hostcheck/cosetmixedcheck.cpp: the planner's invariants, the permutation and offsets, the mixed scalars against slow host_fr.h
    arithmetic and the error order; as a plain program and as a stand-alone ASan + UBSan executable, the same number of checks."""
    plain = _build_and_run(tmp_path, ["-O2"])
    assert re.fullmatch(r"ok \d+\n", plain), plain
    sanitized = _build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert sanitized == plain
