"""CPU checks of the host side of batched header verification: the product-of-pairings predicate for any number of pairs
(`kzg_pairings_product_verify`), the transcript of the batch's weights (`kzg_compute_header_batch_weights`) against a hashlib
restatement, the batch equation itself restated from host entries only, and the declarations of the four new entries.  No GPU."""
import hashlib
import os
import random
import re

import numpy as np
import pytest

import pyref
from pyref import P, R_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    return k


def g1_mul(s):
    return pyref.point_to_wire(pyref.ec_mul(s % R_, (1, 2)) if s % R_ else None)


def g2_mul(k, s):
    return k.helpers.g2_mul_generator(pyref.fr_to_mont(s % R_))


# ---- kzg_pairings_product_verify ----------------------------------------------------------------------------------------------------
def _pairs(k, rnd, count):
    """([a_k]G1, [b_k]G2) with sum a_k b_k = 0 mod r"""
    a = [rnd.randrange(1, R_) for _ in range(count)]
    b = [rnd.randrange(1, R_) for _ in range(count)]
    if count == 1:
        a[0] = 0                                                    # the only way one pair multiplies to 1: an identity
    else:
        partial = sum(x * y for x, y in zip(a[:-1], b[:-1])) % R_
        a[-1] = (-partial) * pow(b[-1], -1, R_) % R_
    return a, b


@pytest.mark.parametrize("count", [1, 2, 4, 5, 9])                  # 5 and 9 cross the 4-pair cap of one shared Miller loop
def test_pairings_product(k, count):
    rnd = random.Random(100 + count)
    a, b = _pairs(k, rnd, count)
    g1s = np.stack([g1_mul(x) for x in a])
    g2s = np.stack([g2_mul(k, y) for y in b])
    assert k.verifier.pairings_product_verify(g1s, g2s) is True
    for pos in {0, count - 1, count // 2}:
        bad = g1s.copy()
        bad[pos] = g1_mul(a[pos] + 1)
        assert k.verifier.pairings_product_verify(bad, g2s) is False, pos
    if count == 2:                                                  # e(a1, a2) e(b1, b2) == 1  <=>  e(a1, a2) == e(-b1, b2)
        neg_b1 = pyref.point_to_wire(pyref.ec_neg(pyref.point_from_wire(g1s[1])))
        assert k.helpers.pairings_verify(g1s[0], g2s[0], neg_b1, g2s[1]) is True
        assert k.helpers.pairings_verify(g1_mul(a[0] + 1), g2s[0], neg_b1, g2s[1]) is False


def test_pairings_product_skips_identities_and_checks_the_curves(k):
    rnd = random.Random(7)
    a, b = _pairs(k, rnd, 5)
    g1s = [g1_mul(x) for x in a]
    g2s = [g2_mul(k, y) for y in b]
    z1, z2 = np.zeros(8, np.uint64), np.zeros(16, np.uint64)
    # identity entries on either side, anywhere, contribute 1: the other five pairs still decide
    g1x = np.stack([z1, g1s[0], g1s[1], g1_mul(5), g1s[2], g1s[3], z1, g1s[4]])
    g2x = np.stack([g2_mul(k, 9), g2s[0], g2s[1], z2, g2s[2], g2s[3], z2, g2s[4]])
    assert k.verifier.pairings_product_verify(g1x, g2x) is True
    g1x[4] = g1_mul(a[2] + 1)
    assert k.verifier.pairings_product_verify(g1x, g2x) is False
    assert k.verifier.pairings_product_verify(np.zeros((0, 8), np.uint64), np.zeros((0, 16), np.uint64)) is True
    off1 = np.stack(g1s); off1[3, 0] ^= np.uint64(1)
    with pytest.raises(k.errors.NotOnCurveError, match="G1"):
        k.verifier.pairings_product_verify(off1, np.stack(g2s))
    off2 = np.stack(g2s); off2[4, 9] ^= np.uint64(4)
    with pytest.raises(k.errors.NotOnCurveError, match="G2"):
        k.verifier.pairings_product_verify(np.stack(g1s), off2)
    with pytest.raises(k.errors.NotOnCurveError, match="G1"):       # both: every G1 input is tested first
        k.verifier.pairings_product_verify(off1, off2)


# ---- the weights ----------------------------------------------------------------------------------------------------------------------
def _g2bytes(k, pt):
    pt = np.asarray(pt, np.uint64).reshape(16)
    if not pt.any():
        return bytes(128)
    return b"".join(pyref.fq_from_mont(pt[4 * j:4 * j + 4]).to_bytes(32, "big") for j in range(4))


def weights_py(k, commitments, c2s, pi2s, lens, shifts):
    """the transcript of include/kzg_bn254_mi355x.h (kzg_compute_header_batch_weights), restated"""
    count = len(commitments)
    parts = [b"KZGBN254_HEADERBATCH_V1_", count.to_bytes(8, "big"), len(shifts).to_bytes(8, "big")]
    for d, pt in shifts.items():
        parts += [int(d).to_bytes(8, "big"), k.helpers.serialize_compressed(pt)]
    for i in range(count):
        item = b"KZGBN254_HEADERITEM__V1_" + int(lens[i]).to_bytes(8, "big") + k.helpers.serialize_compressed(commitments[i])
        item += _g2bytes(k, c2s[i]) + _g2bytes(k, pi2s[i])
        parts.append(hashlib.sha256(item).digest())
    seed = hashlib.sha256(b"".join(parts)).digest()
    return [int.from_bytes(hashlib.sha256(seed + j.to_bytes(8, "big")).digest()[:16], "big") for j in range(count + 1)]


def _headers(k, rnd, tau, N, lens):
    """honest headers from a known tau: scalars f_i, and (C, C2, pi2) = ([f]_1, [f]_2, [tau^(N-d) f]_2)"""
    fs = [rnd.randrange(1, R_) for _ in lens]
    c = np.stack([g1_mul(f) for f in fs])
    c2 = np.stack([g2_mul(k, f) for f in fs])
    pi2 = np.stack([g2_mul(k, pow(tau, N - d, R_) * f) for f, d in zip(fs, lens)])
    return fs, c, c2, pi2


@pytest.mark.parametrize("count", [0, 1, 3])
def test_weights_match_the_restated_transcript(k, count):
    rnd = random.Random(200 + count)
    tau, N = 0x1234567, 16
    lens = [4, 16, 4][:count]
    shifts = {d: g1_mul(pow(tau, N - d, R_)) for d in (4, 16)}
    _, c, c2, pi2 = _headers(k, rnd, tau, N, lens) if count else (None, np.zeros((0, 8), np.uint64), np.zeros((0, 16), np.uint64), np.zeros((0, 16), np.uint64))
    if count == 3:                                                  # an identity G2 point among them, and an identity commitment
        c2[1] = 0
        c[2] = 0
    got = k.verifier.compute_header_batch_weights(c, c2, pi2, lens, shifts)
    want = weights_py(k, c, c2, pi2, lens, shifts)
    assert got.shape == (count + 1, 4)
    assert pyref.frs_from_mont(got) == want
    assert all(w < 2 ** 128 for w in want)
    assert len(set(want)) == count + 1
    if count:                                                       # every input is bound: one changed length changes every weight
        other = k.verifier.compute_header_batch_weights(c, c2, pi2, [16] + lens[1:], shifts)
        assert all(a != b for a, b in zip(pyref.frs_from_mont(other), want))


# ---- the equation -------------------------------------------------------------------------------------------------------------------
def _batch_equation(k, fs, pis, lens, shifts_scalar, weights):
    """e(U, G2) e(-G1, S + [rho]Pi) prod_g e([rho]T_g, W_g) == 1 with every group element made from its known scalar by host entries:
    header i is ([f_i]_1, [f_i]_2, [pi_i]_2), T_g = [shifts_scalar[g]]_1"""
    r, rho = weights[:-1], weights[-1]
    U = g1_mul(sum(ri * f for ri, f in zip(r, fs)))
    groups = sorted(set(lens))
    Ws = {d: sum(ri * f for ri, f, di in zip(r, fs, lens) if di == d) % R_ for d in groups}
    S = sum(Ws.values()) % R_
    Pi = sum(ri * p for ri, p in zip(r, pis)) % R_
    neg_g1 = pyref.point_to_wire(pyref.ec_neg((1, 2)))
    g1s = [U, neg_g1] + [g1_mul(rho * shifts_scalar[d]) for d in groups]
    g2s = [g2_mul(k, 1), g2_mul(k, S + rho * Pi)] + [g2_mul(k, Ws[d]) for d in groups]
    return k.verifier.pairings_product_verify(np.stack(g1s), np.stack(g2s))


def test_batch_equation_restated_from_host_entries(k):
    rnd = random.Random(300)
    tau, N = rnd.randrange(2, R_), 16
    lens = [4, 16, 4, 4, 16]                                        # 5 headers in 2 groups
    shifts_scalar = {d: pow(tau, N - d, R_) for d in (4, 16)}
    shifts = {d: g1_mul(s) for d, s in shifts_scalar.items()}
    fs, c, c2, pi2 = _headers(k, rnd, tau, N, lens)
    pis = [shifts_scalar[d] * f % R_ for f, d in zip(fs, lens)]
    w = pyref.frs_from_mont(k.verifier.compute_header_batch_weights(c, c2, pi2, lens, shifts))
    assert _batch_equation(k, fs, pis, lens, shifts_scalar, w) is True
    # one pi2 off by G2: the weights are derived from the tampered header, as a verifier would
    bad_pi2 = pi2.copy()
    bad_pi2[3] = g2_mul(k, pis[3] + 1)
    wb = pyref.frs_from_mont(k.verifier.compute_header_batch_weights(c, c2, bad_pi2, lens, shifts))
    assert _batch_equation(k, fs, pis[:3] + [pis[3] + 1] + pis[4:], lens, shifts_scalar, wb) is False
    # every honest header passes the single-call check the batch is measured against
    for i in range(5):
        assert k.verifier.verify_length_proof(c[i], c2[i], pi2[i], shifts[lens[i]]) is True
    assert k.verifier.verify_length_proof(c[3], c2[3], bad_pi2[3], shifts[4]) is False


# ---- declarations ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_as_the_prototypes_do(k):
    hdr = open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read()
    L = k._lib
    i32p, u64o = L.C.POINTER(L.i32), L.C.POINTER(L.C.c_uint64)
    want = {
        "kzg_pairings_product_verify": (["g1s_xy", "g2s", "count", "out_ok"], [L.u64p, L.u64p, L.sz, i32p]),
        "kzg_g2_check_subgroup": (["ctx", "g2_mont", "n_points", "bad_index"], [L.vp, L.u64p, L.sz, u64o]),
        "kzg_compute_header_batch_weights": (["commitments_xy", "length_commitments", "length_proofs", "claimed_lens", "count", "shift_lens", "g1_tau_shifts_xy",
                                              "n_shifts", "out_weights_mont"], [L.u64p, L.u64p, L.u64p, L.u64p, L.sz, L.u64p, L.u64p, L.sz, L.u64p]),
        "kzg_verify_length_proof_batch": (["ctx", "commitments_xy", "length_commitments", "length_proofs", "claimed_lens", "count", "shift_lens", "g1_tau_shifts_xy",
                                           "n_shifts", "weights_mont", "out_ok", "bad_index"],
                                          [L.vp, L.u64p, L.u64p, L.u64p, L.u64p, L.sz, L.u64p, L.u64p, L.sz, L.u64p, i32p, u64o]),
    }
    import ctypes as C
    lib = C.CDLL(L.LIB_PATH)
    for name, (params, argtypes) in want.items():
        decl = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert decl, name + " is not declared"
        text = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S)
        assert [p.split()[-1] for p in text.split(",")] == params, name
        assert L.PROTOTYPES[name] == (L.i32, argtypes), name
        assert hasattr(lib, name)
    hpp = open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.hpp")).read()
    for name in want:
        if name != "kzg_compute_header_batch_weights":
            assert name + "(" in hpp, name


def test_python_argument_errors_need_no_device(k):
    with pytest.raises(k.errors.InvalidInputLength):
        k.verifier.verify_length_proof_batch(np.zeros((2, 8), np.uint64), np.zeros((1, 16), np.uint64), np.zeros((2, 16), np.uint64), [4, 4], {4: g1_mul(1)})
    with pytest.raises(k.errors.InvalidInputLength):
        k.verifier.pairings_product_verify(np.zeros((2, 8), np.uint64), np.zeros((1, 16), np.uint64))
