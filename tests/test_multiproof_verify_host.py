"""CPU-only checks of the verification of coset proofs (`kzg_verify_multiproof`, `kzg_verify_multiproof_batch`): the batch equation
restated over Fr with a known tau, the Fiat-Shamir transcript of `kzg_compute_multiproof_r_powers` (host-only C) against its Python twin
and a hand-assembled one, the declarations of the four entries, the argument errors that need no device, and the decoder of the
mainnet G2 powers."""
import ctypes as C
import hashlib
import os
import random
import re

import numpy as np
import pytest

import coset_ref
import pyref
from pyref import R_, dft, poly_eval, root_of_unity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRIES = ("kzg_coset_interpolate_rlc", "kzg_compute_multiproof_r_powers", "kzg_verify_multiproof_batch", "kzg_verify_multiproof")


def quotient_at(f, l, c, tau):
    """[f / (X^l - c)](tau), the remainder dropped"""
    f = list(f)
    q = [0] * (len(f) - l)
    for i in range(len(f) - 1, l - 1, -1):
        q[i - l] = f[i]
        f[i - l] = (f[i - l] + f[i] * c) % R_
    return poly_eval(q, tau)


@pytest.mark.parametrize("l", [1, 2, 8, 64])
def test_fast_ifft_of_the_reference_is_the_definition(l):
    rnd = random.Random(l)
    v = [rnd.randrange(R_) for _ in range(l)]
    assert coset_ref.ifft(v) == dft(v, inverse=True)


@pytest.mark.parametrize("log_n,l", [(6, 1), (6, 4), (8, 16), (5, 16)])
def test_batch_equation_over_fr_with_a_known_tau(log_n, l):
    """Setup: tau known, group elements as their discrete logarithms.  3 polynomials, 10 items with a repeated item and mixed rows;
    the equation holds, and fails when one y, one proof, one coset index or one row index is changed.  Pins the sign and direction of
    the twist w^(-k t) and the natural-order IFFT with root w^m."""
    n, m = 1 << log_n, (1 << log_n) // l
    rnd = random.Random(1000 * log_n + l)
    tau = rnd.randrange(2, R_)
    w = root_of_unity(log_n)
    assert pow(w, m, R_) == root_of_unity(l.bit_length() - 1)                   # w^m is the root IFFT_l runs over
    polys = [[rnd.randrange(R_) for _ in range(n)] for _ in range(3)]
    evals = [dft(f) for f in polys]
    commitments = [poly_eval(f, tau) for f in polys]
    rows = [rnd.randrange(3) for _ in range(10)]
    ks = [rnd.randrange(m) for _ in range(10)]
    rows[7], ks[7] = rows[2], ks[2]                                            # the same item twice
    assert len(set(rows)) > 1
    ys = [evals[c][k::m] for c, k in zip(rows, ks)]
    for c, k, y in zip(rows, ks, ys):
        assert len(y) == l
        coeffs = coset_ref.interpolation_coeffs(y, k, n)
        for j in range(l):                                                     # I_k interpolates the coset
            assert poly_eval(coeffs, pow(w, k + j * m, R_)) == y[j]
    proofs = [quotient_at(polys[c], l, pow(w, k * l, R_), tau) for c, k in zip(rows, ks)]
    r = rnd.randrange(R_)
    weights = [pow(r, i, R_) for i in range(10)]
    assert coset_ref.batch_equation_holds(tau, n, l, commitments, rows, ks, ys, proofs, weights)
    # one item alone, weight 1: e(pi, [tau^l - h^l]) = e(C - I(tau), G2)
    i0 = 4
    I_tau = poly_eval(coset_ref.interpolation_coeffs(ys[i0], ks[i0], n), tau)
    assert proofs[i0] * (pow(tau, l, R_) - pow(w, ks[i0] * l, R_)) % R_ == (commitments[rows[i0]] - I_tau) % R_
    assert coset_ref.batch_equation_holds(tau, n, l, commitments, [rows[i0]], [ks[i0]], [ys[i0]], [proofs[i0]], [1])
    bad_y = [list(y) for y in ys]
    bad_y[3][l - 1] = (bad_y[3][l - 1] + 1) % R_
    assert not coset_ref.batch_equation_holds(tau, n, l, commitments, rows, ks, bad_y, proofs, weights)
    bad_p = list(proofs)
    bad_p[5] = (bad_p[5] + 1) % R_
    assert not coset_ref.batch_equation_holds(tau, n, l, commitments, rows, ks, ys, bad_p, weights)
    bad_k = list(ks)
    bad_k[6] = (bad_k[6] + 1) % m
    assert not coset_ref.batch_equation_holds(tau, n, l, commitments, rows, bad_k, ys, proofs, weights)
    bad_c = list(rows)
    bad_c[1] = (bad_c[1] + 1) % 3
    assert not coset_ref.batch_equation_holds(tau, n, l, commitments, bad_c, ks, ys, proofs, weights)


def _random_point(rnd):
    return pyref.point_to_wire(pyref.ec_mul(rnd.randrange(1, R_), (1, 2)))


@pytest.mark.parametrize("count", [1, 2, 33, 300])
@pytest.mark.parametrize("l", [1, 4])
def test_r_powers_c_abi_matches_python_twin_and_hand_built_transcript(count, l):
    """`kzg_compute_multiproof_r_powers` (host only, item digests on the host pool) against `compute_multiproof_r_powers_py` and a
    transcript assembled here with hashlib: identity points, y = 0 and y = r - 1; changing any single input changes r."""
    import rust_kzg_bn254_amd as k
    from rust_kzg_bn254_amd import verifier
    rnd = random.Random(17 * count + l)
    n, M = 64, 3
    pool = [_random_point(rnd) for _ in range(4)] + [np.zeros(8, np.uint64)]
    commitments = [pool[0], pool[4], pool[1]]                                  # one identity commitment
    proofs = [pool[rnd.randrange(5)] for _ in range(count)]
    proofs[0] = pool[4]                                                        # an identity proof
    rows = [rnd.randrange(M) for _ in range(count)]
    ks = [rnd.randrange(n // l) for _ in range(count)]
    y_int = [[rnd.randrange(R_) for _ in range(l)] for _ in range(count)]
    y_int[0][0] = 0
    y_int[-1][l - 1] = R_ - 1
    ys = np.stack([pyref.frs_to_mont(v) for v in y_int])
    got = verifier.compute_multiproof_r_powers(commitments, rows, ks, ys, proofs, n)
    twin = verifier.compute_multiproof_r_powers_py(commitments, rows, ks, ys, proofs, n)
    assert np.array_equal(got, twin)

    def compressed(p):
        pt = pyref.point_from_wire(p)
        if pt is None:
            return bytes(31) + b"\x40"
        b = bytearray(pt[0].to_bytes(32, "little"))
        if pt[1] > (pyref.P - 1) // 2:
            b[31] |= 0x80
        return bytes(b)

    data = b"KZGBN254_COSETBATCH__V1_" + n.to_bytes(8, "big") + l.to_bytes(8, "big") + M.to_bytes(8, "big") + count.to_bytes(8, "big")
    data += b"".join(compressed(c) for c in commitments)
    for i in range(count):
        item = b"KZGBN254_COSETITEM___V1_" + rows[i].to_bytes(8, "big") + ks[i].to_bytes(8, "big")
        item += b"".join(v.to_bytes(32, "big") for v in y_int[i]) + compressed(proofs[i])
        assert len(item) == 24 + 16 + 32 * l + 32
        data += hashlib.sha256(item).digest()
    r = int.from_bytes(hashlib.sha256(data).digest(), "big") % R_
    assert pyref.frs_from_mont(got) == [pow(r, i, R_) for i in range(count)]
    if count < 2:
        return

    def r_of(**kw):
        a = dict(commitments=commitments, rows=rows, ks=ks, ys=ys, proofs=proofs, n=n)
        a.update(kw)
        return pyref.fr_from_mont(verifier.compute_multiproof_r_powers(a["commitments"], a["rows"], a["ks"], a["ys"], a["proofs"], a["n"])[1])

    assert r_of() == r
    seen = {r}
    ys2 = ys.copy(); ys2[count - 1, l - 1] = pyref.fr_to_mont(5)
    rows2 = list(rows); rows2[1] = (rows2[1] + 1) % M
    ks2 = list(ks); ks2[count - 1] = (ks2[count - 1] + 1) % (n // l)
    proofs2 = list(proofs); proofs2[count - 1] = pool[0] if proofs[count - 1] is not pool[0] else pool[1]
    commitments2 = [pool[0], pool[4], pool[2]]
    for kw in (dict(ys=ys2), dict(rows=rows2), dict(ks=ks2), dict(proofs=proofs2), dict(commitments=commitments2), dict(n=128)):
        v = r_of(**kw)
        assert v not in seen, kw.keys()
        seen.add(v)
    assert len(k.verifier.compute_multiproof_r_powers(commitments, [], [], np.zeros((0, l, 4), np.uint64), [], n)) == 0


def test_header_prototypes_and_exports_agree_on_the_four_entries():
    import rust_kzg_bn254_amd as k
    hdr = open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read()
    lib = C.CDLL(k._lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint32_t %s\s*\(" % name, hdr), name
        assert name in k._lib.PROTOTYPES, name
        assert hasattr(lib, name), name
    u64p, vp, sz, i32 = k._lib.u64p, k._lib.vp, k._lib.sz, k._lib.i32
    assert k._lib.PROTOTYPES["kzg_coset_interpolate_rlc"] == (i32, [vp, u64p, u64p, u64p, sz, sz, sz, u64p])
    assert k._lib.PROTOTYPES["kzg_compute_multiproof_r_powers"] == (i32, [u64p, sz, u64p, u64p, u64p, u64p, sz, sz, sz, u64p])
    assert k._lib.PROTOTYPES["kzg_verify_multiproof_batch"] == (i32, [vp, vp, u64p, sz, u64p, u64p, u64p, u64p, sz, sz, sz, u64p, u64p, C.POINTER(i32)])
    assert k._lib.PROTOTYPES["kzg_verify_multiproof"] == (i32, [vp, vp, u64p, u64p, C.c_uint64, u64p, sz, sz, u64p, C.POINTER(i32)])
    # argument counts of the header's declarations
    for name in ENTRIES:
        decl = re.search(r"\bint32_t %s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(k._lib.PROTOTYPES[name][1]), name


class _FakeSrs:
    handle = None

    def __len__(self):
        return 64


def test_argument_errors_that_need_no_device():
    """Null pointers and a NULL g2_tau_l with l = 2 through the C-ABI (no context exists: every call returns before it needs one), and
    the same through the Python surface, which must not create a context for them."""
    import rust_kzg_bn254_amd as k
    from rust_kzg_bn254_amd import verifier
    lib = k.load()
    L = k._lib
    ok = L.i32(7)
    one = pyref.frs_to_mont([1])
    pt = np.zeros((1, 8), np.uint64)
    idx = np.zeros(1, np.uint64)
    ys = np.zeros((1, 2, 4), np.uint64)
    g2 = k.helpers.g2_generator()
    assert lib.kzg_verify_multiproof_batch(None, None, L.ptr(pt), 1, L.ptr(idx), L.ptr(idx), L.ptr(ys), L.ptr(pt), 1, 8, 2, L.ptr(one), L.ptr(g2), C.byref(ok)) == L.ERR_INVALID_ARG
    assert lib.kzg_verify_multiproof(None, None, L.ptr(pt), L.ptr(pt), 0, L.ptr(ys), 8, 2, None, C.byref(ok)) == L.ERR_INVALID_ARG
    assert lib.kzg_verify_multiproof(None, None, None, L.ptr(pt), 0, L.ptr(ys), 8, 2, L.ptr(g2), C.byref(ok)) == L.ERR_INVALID_ARG
    assert lib.kzg_coset_interpolate_rlc(None, L.ptr(ys), L.ptr(idx), L.ptr(one), 1, 8, 2, L.ptr(ys)) == L.ERR_INVALID_ARG
    assert ok.value == 7
    out = np.zeros((1, 4), np.uint64)
    assert lib.kzg_compute_multiproof_r_powers(L.ptr(pt), 1, None, L.ptr(idx), L.ptr(ys), L.ptr(pt), 1, 8, 2, L.ptr(out)) == L.ERR_INVALID_ARG
    assert lib.kzg_compute_multiproof_r_powers(L.ptr(pt), 1, L.ptr(idx), L.ptr(idx), L.ptr(ys), L.ptr(pt), 1, 8, 2, None) == L.ERR_INVALID_ARG
    assert lib.kzg_compute_multiproof_r_powers(None, 0, None, None, None, None, 0, 8, 2, None) == L.OK
    before = dict(k._lib._default_ctx)                                          # device id -> Context: must not grow
    with pytest.raises(k.errors.GenericError, match="tau\\^l"):
        verifier.verify_multiproof_batch([pt[0]], [0], [0], ys, [pt[0]], 8, _FakeSrs(), g2_tau_l=None)
    with pytest.raises(k.errors.GenericError, match="tau\\^l"):
        verifier.verify_multiproof(pt[0], pt[0], 0, ys[0], 8, _FakeSrs(), g2_tau_l=None)
    with pytest.raises(k.errors.GenericError, match="not the same"):
        verifier.verify_multiproof_batch([pt[0]], [0, 0], [0], ys, [pt[0]], 8, _FakeSrs(), g2_tau_l=g2)
    with pytest.raises(k.errors.InvalidInputLength):
        verifier.verify_multiproof_batch([pt[0]], [0], [0], np.zeros((1, 8), np.uint64), [pt[0]], 8, _FakeSrs(), g2_tau_l=g2)
    assert k._lib._default_ctx == before


def test_cosets_layout_matches_the_proof_rows():
    import rust_kzg_bn254_amd as k
    ev = pyref.frs_to_mont(list(range(100, 164)))
    poly = k.PolynomialEvalForm(ev)
    kzg = k.KZG.new()
    for l in (1, 4, 32):
        m = 64 // l
        c = kzg.cosets(poly, l)
        assert c.shape == (m, l, 4) and c.flags["C_CONTIGUOUS"]
        for kk in (0, 1, m - 1):
            assert np.array_equal(c[kk], ev[kk::m])
    with pytest.raises(k.errors.GenericError):
        kzg.cosets(poly, 3)
    with pytest.raises(k.errors.GenericError):
        kzg.cosets(poly, 64)
    assert kzg.ctx is None


def test_read_g2_powers_of_2_on_the_mainnet_fixture(tmp_path):
    """tests/golden/g2.point.powerOf2 (the reference's mainnet file): 28 distinct points, entry 0 = consts::G2_TAU, every entry valid
    for `kzg_validate_g2_point` (on the twist, finite, in the order-r subgroup, not the generator).  That entry i really is
    [tau^(2^i)]_2 cannot be checked here: the fixtures hold no G1 powers of the mainnet tau."""
    import rust_kzg_bn254_amd as k
    path = os.path.join(GOLDEN, "g2.point.powerOf2")
    pts = k.helpers.read_g2_powers_of_2(path)
    assert pts.shape == (28, 16) and pts.dtype == np.uint64
    assert len({p.tobytes() for p in pts}) == 28
    assert np.array_equal(pts[0], k.helpers.g2_tau())
    lib = k.load()
    for p in pts:
        reason = k._lib.i32(9)
        assert lib.kzg_validate_g2_point(k._lib.ptr(np.ascontiguousarray(p)), C.byref(reason)) == 0 and reason.value == 0
    data = open(path, "rb").read()
    short = tmp_path / "short"
    short.write_bytes(data[:100])
    with pytest.raises(k.errors.DeserializationError):
        k.helpers.read_g2_powers_of_2(str(short))
    flagged = tmp_path / "flag"
    flagged.write_bytes(bytes([data[0] & 0x3F]) + data[1:64])                  # flag bits 0b00: an uncompressed point in gnark's encoding
    with pytest.raises(k.errors.DeserializationError):
        k.helpers.read_g2_powers_of_2(str(flagged))
    empty = tmp_path / "empty"
    empty.write_bytes(b"")
    with pytest.raises(k.errors.DeserializationError):
        k.helpers.read_g2_powers_of_2(str(empty))
