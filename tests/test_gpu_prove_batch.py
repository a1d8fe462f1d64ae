"""-m gpu: the batched prover (kzg_compute_proof_batch, kzg_compute_blob_proof_batch, kzg_commit_and_prove_blob_batch): many proofs in one
call -- one fused evaluate-and-divide kernel (a workgroup per polynomial of up to 2^12 evaluations, points on the domain included) and one
batched MSM over the cached Lagrange basis.  No counterpart in the reference, which proves one polynomial per call (prover/src/kzg.rs:128-178,
:288-309): every row must equal the single call bit for bit, the reference's golden proofs, the oracle and known-tau values."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import oracle as orc
import pyref
from pyref import R_

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
TAU = int.from_bytes(__import__("hashlib").sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % R_


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


@pytest.fixture(scope="module")
def tau_srs(k):
    s = k.SRS.generate(TAU, 1 << 13)
    yield s
    s.close()


@pytest.fixture(scope="module")
def ref_srs(k, test_srs_wire):
    s = k.SRS(test_srs_wire, order=3000)
    yield s
    s.close()


def special_points(n, rnd):
    """a random point, w^0, w^(n-1), w^(n/2), 0"""
    w = pyref.root_of_unity(n.bit_length() - 1)
    return [rnd.randrange(R_), 1, pow(w, n - 1, R_), pow(w, n // 2, R_), 0]


def single_kzg(k, n):
    kzg = k.KZG.new()
    kzg.calculate_and_store_roots_of_unity(n * 32)
    return kzg


def eval_at(f, x, n):
    """f(x) of the polynomial with the values f on the n-point domain, x off the domain: the barycentric formula in big integers"""
    w = pyref.root_of_unity(n.bit_length() - 1)
    total, wj = 0, 1
    for j in range(n):
        total = (total + f[j] * wj % R_ * pow(x - wj, -1, R_)) % R_
        wj = wj * w % R_
    return (pow(x, n, R_) - 1) * pow(n, -1, R_) % R_ * total % R_


def test_golden_rows_in_one_call(k, ref_srs, gettysburg):
    """All 40 rows of kzg.proof.eq.input (z = the row's root of unity, kzg.rs:237-260) in ONE call."""
    blob = k.Blob.from_raw_data(gettysburg)
    poly = blob.to_polynomial_eval_form()
    kzg = k.KZG.new(); kzg.calculate_and_store_roots_of_unity(len(blob))
    rows = [line.strip().split(",") for line in open(os.path.join(GOLDEN, "kzg.proof.eq.input")) if line.strip()]
    assert len(rows) == 40
    zs = [kzg.get_nth_root_of_unity(int(idx)) for idx, _, _ in rows]
    got, ys = kzg.compute_proof_batch([poly] * len(rows), zs, ref_srs, want_y=True)
    assert got.shape == (40, 8)
    ev = poly.evaluations()
    for j, (idx, x, y) in enumerate(rows):
        assert pyref.point_from_wire(got[j]) == (int(x), int(y)), idx
        assert np.array_equal(got[j], kzg.compute_proof(poly, zs[j], ref_srs)), idx
        assert np.array_equal(ys[j], ev[int(idx)]), idx


@pytest.mark.parametrize("log_n", range(13))
def test_every_size_equals_single_calls_and_oracle(k, tau_srs, log_n):
    """Every power of two up to 2^12: Lf < 64 lanes, a whole workgroup, and 2 / 4 / 8 elements per lane; 5 polynomials per size at a random
    point, w^0, w^(n-1), w^(n/2) and 0."""
    n = 1 << log_n
    rnd = random.Random(4000 + log_n)
    polys = [k.PolynomialEvalForm(pyref.frs_to_mont([rnd.randrange(R_) for _ in range(n)])) for _ in range(5)]
    zs = [pyref.fr_to_mont(z) for z in special_points(n, rnd)]
    kzg = single_kzg(k, n)
    got, ys = kzg.compute_proof_batch(polys, zs, tau_srs, want_y=True)
    srs_wire = tau_srs.g1[:n]
    count, roots = orc.calculate_roots_of_unity(n * 32)
    assert count == n
    for p, z, g, y in zip(polys, zs, got, ys):
        one, one_y = kzg._compute_proof_impl(p, z, tau_srs, want_y=True)
        assert np.array_equal(g, one) and np.array_equal(y, one_y), log_n
        rc, want, want_y = orc.compute_proof(srs_wire, p.evaluations(), roots, z, literal=False)
        assert rc == 0 and np.array_equal(g, want) and np.array_equal(y, want_y), log_n


def test_many_polynomials_known_tau(k, tau_srs):
    """1 030 polynomials of 512 evaluations (two launches of the batched MSM: 1 024 + 6) on a known-tau SRS; every eighth row special (zero,
    one-hot, all r - 1, all 1, the recoder's digit patterns), the points random, on the domain and 0: the first 40 rows and the last 30
    against [(f(tau) - y) / (tau - z)] G by big-integer arithmetic."""
    kzg = k.KZG.new()
    n, count = 512, 1030
    rnd = random.Random(9)
    w = pyref.root_of_unity(9)
    rows, zs = [], []
    for j in range(count):
        kind = j % 8
        if kind == 0:
            v = [0] * n
        elif kind == 1:
            v = [0] * n; v[(j * 37) % n] = rnd.randrange(R_)
        elif kind == 2:
            v = [R_ - 1] * n
        elif kind == 3:
            v = [1] * n
        elif kind == 4:
            v = [(1 << 253) - 1 if i % 2 == 0 else (1 << 36) - 1 for i in range(n)]
        else:
            v = [rnd.randrange(R_) for _ in range(n)]
        rows.append(v)
        zs.append(pow(w, (j * 37) % n, R_) if j % 5 == 1 else 0 if j % 5 == 3 else rnd.randrange(R_))
    data = np.stack([pyref.frs_to_mont(v) for v in rows])
    got, ys = kzg.compute_proof_batch(data, [pyref.fr_to_mont(z) for z in zs], tau_srs, want_y=True)
    for j in list(range(0, 40)) + list(range(1000, count)):
        z = zs[j]
        y = rows[j][(j * 37) % n] if j % 5 == 1 else eval_at(rows[j], z, n)
        assert pyref.fr_from_mont(ys[j]) == y, j
        s = (eval_at(rows[j], TAU, n) - y) * pow(TAU - z, -1, R_) % R_
        want = pyref.ec_mul(s, (1, 2)) if s else None
        assert pyref.point_from_wire(got[j]) == want, j
    single = single_kzg(k, n)
    for j in range(0, count, 97):                                                       # and single calls at a stride
        assert np.array_equal(got[j], single._compute_proof_impl(k.PolynomialEvalForm(data[j]), pyref.fr_to_mont(zs[j]), tau_srs)), j


def mixed_blobs(k, gettysburg):
    """31 B, 32 B, 33 B, 1 000 B, the Gettysburg fixture, 2^12 elements exactly, 2^12 + 1 elements (the single-proof branch)"""
    rnd = random.Random(77)

    def elems(count, tail=0):
        return b"".join(b"\x00" + bytes(rnd.randrange(256) for _ in range(31)) for _ in range(count)) + b"\x00" * bool(tail) + bytes(rnd.randrange(256) for _ in range(max(tail - 1, 0)))
    datas = [elems(0, 31), elems(1), elems(1, 1), elems(31, 8), None, elems(4096), elems(4097)]
    assert [len(d) for d in datas if d is not None] == [31, 32, 33, 1000, 4096 * 32, 4097 * 32]
    return [k.Blob.from_raw_data(gettysburg) if d is None else k.Blob.from_padded_unchecked(d) for d in datas]


@pytest.fixture(scope="module")
def mixed(k, tau_srs, gettysburg):
    """the mixed blobs with their single-call results, computed once"""
    blobs = mixed_blobs(k, gettysburg)
    singles = []
    for b in blobs:
        kzg = k.KZG.new(); kzg.calculate_and_store_roots_of_unity(len(b.data()))
        singles.append(kzg.commit_and_prove_blob(b, tau_srs))
    return blobs, singles


def test_mixed_lengths_in_one_bytes_call(k, tau_srs, mixed):
    blobs, singles = mixed
    kzg = k.KZG.new()
    com, proofs, zs, ys = kzg.commit_and_prove_blob_batch(blobs, tau_srs)
    for j, (c1, p1, z1, y1) in enumerate(singles):
        assert np.array_equal(com[j], c1) and np.array_equal(proofs[j], p1) and np.array_equal(zs[j], z1) and np.array_equal(ys[j], y1), j
    p2, z2, y2 = kzg.compute_blob_proof_batch(blobs, com, tau_srs, want_zy=True)
    assert np.array_equal(p2, proofs) and np.array_equal(z2, zs) and np.array_equal(y2, ys)
    for j, b in enumerate(blobs):
        one = k.KZG.new(); one.calculate_and_store_roots_of_unity(len(b.data()))
        assert np.array_equal(p2[j], one.compute_blob_proof(b, com[j], tau_srs)), j
    g2_tau = k.helpers.g2_mul_generator(k.fr.fr_from_int(TAU))
    assert k.verifier.verify_blob_kzg_proof_batch(blobs, list(com), list(proofs), g2_tau)
    changed = bytearray(blobs[3].data()); changed[40] ^= 1
    tampered = blobs[:3] + [k.Blob.from_padded_unchecked(bytes(changed))] + blobs[4:]
    assert not k.verifier.verify_blob_kzg_proof_batch(tampered, list(com), list(proofs), g2_tau)


def test_group_budget_does_not_change_a_byte(k, tau_srs, mixed, gettysburg):
    """The budget shrunk so that every class splits into groups of one row: identical bytes."""
    rnd = random.Random(5)
    blobs = mixed[0][:5] * 3                                                            # three blobs in each of four classes (31 / 32 B share one)
    polys = [k.PolynomialEvalForm(pyref.frs_to_mont([rnd.randrange(R_) for _ in range(1024)])) for _ in range(5)]
    pz = [pyref.fr_to_mont(z) for z in special_points(1024, rnd)]
    kzg = k.KZG.new()
    ctx = tau_srs.ctx
    want = kzg.commit_and_prove_blob_batch(blobs, tau_srs)
    want_p = kzg.compute_proof_batch(polys, pz, tau_srs, want_y=True)
    try:
        for budget in (1, 3 * 1024 * 96):
            ctx.set_prove_group_bytes(budget)
            got = kzg.commit_and_prove_blob_batch(blobs, tau_srs)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), budget
            got_p = kzg.compute_proof_batch(polys, pz, tau_srs, want_y=True)
            assert all(np.array_equal(a, b) for a, b in zip(got_p, want_p)), budget
    finally:
        ctx.set_prove_group_bytes(0)
    with pytest.raises(ValueError):
        ctx.set_prove_group_bytes(-1)


def test_error_rows(k, tau_srs, ref_srs, mixed):
    L = k._lib
    lib = L.load()
    ctx = tau_srs.ctx
    kzg = k.KZG.new()
    blobs = list(mixed[0][:5]) + [k.Blob.from_padded_unchecked(b""), mixed[0][0]]
    com = [c for c, _, _, _ in mixed[1][:5]] + [mixed[1][0][0], mixed[1][0][0]]
    off = np.array(com[3], dtype=np.uint64); off[0] ^= 1
    # an off-curve commitment at index 3 and an empty blob at index 5: index 3 is reported
    ptrs, lens, keep = L.blob_args(blobs)
    cm = np.ascontiguousarray(np.stack(com[:3] + [off] + com[4:]), dtype=np.uint64)
    out = np.full((7, 8), 0x5A, dtype=np.uint64); bad = C.c_size_t(99)
    rc = lib.kzg_compute_blob_proof_batch(ctx.handle, tau_srs.handle, ptrs, lens, L.ptr(cm), 7, L.ptr(out), None, None, None, C.byref(bad))
    assert rc == L.ERR_G1_NOT_ON_CURVE and bad.value == 3 and (out == 0x5A).all()
    with pytest.raises(k.errors.NotOnCurveError):
        kzg.compute_blob_proof_batch(blobs, list(cm), tau_srs)
    rc = lib.kzg_compute_blob_proof_batch(ctx.handle, tau_srs.handle, ptrs, lens, L.ptr(np.ascontiguousarray(np.stack(com))), 7, L.ptr(out), None, None, None, C.byref(bad))
    assert rc == L.ERR_ZERO_LENGTH and bad.value == 5
    with pytest.raises(k.errors.GenericError):
        kzg.commit_and_prove_blob_batch(blobs, tau_srs)
    # count = 0: nothing written
    assert lib.kzg_compute_blob_proof_batch(ctx.handle, tau_srs.handle, None, None, None, 0, L.ptr(out), None, None, None, C.byref(bad)) == L.OK
    assert (out == 0x5A).all() and bad.value == 5
    assert kzg.commit_and_prove_blob_batch([], tau_srs)[1].shape == (0, 8)
    # a class larger than the SRS (3000 points: 2^12 elements do not fit)
    with pytest.raises(k.errors.SrsCapacityExceeded):
        kzg.commit_and_prove_blob_batch(list(mixed[0][:6]), ref_srs)
    ptrs6, lens6, keep6 = L.blob_args(mixed[0][:6])
    bad.value = 99
    rc = lib.kzg_commit_and_prove_blob_batch(ref_srs.ctx.handle, ref_srs.handle, ptrs6, lens6, 6, L.ptr(out), None, L.ptr(out), None, None, None, C.byref(bad))
    assert rc == L.ERR_SRS_CAPACITY_EXCEEDED and bad.value == 5
    ev = np.zeros((2, 4096, 4), dtype=np.uint64); z2 = np.zeros((2, 4), dtype=np.uint64)
    assert lib.kzg_compute_proof_batch(ref_srs.ctx.handle, ref_srs.handle, L.ptr(ev), 4096, 2, L.ptr(z2), L.ptr(out), None, None) == L.ERR_SRS_CAPACITY_EXCEEDED
    assert lib.kzg_compute_proof_batch(ctx.handle, tau_srs.handle, L.ptr(ev), 48, 2, L.ptr(z2), L.ptr(out), None, None) == L.ERR_INVALID_INPUT_LENGTH
    # a kzg_*_begin in flight: refused, and the context is usable afterwards
    data = np.frombuffer(mixed[0][3].data(), dtype=np.uint8)
    assert lib.kzg_commit_blob_begin(ctx.handle, tau_srs.handle, data.ctypes.data_as(L.u8p), len(data), 1) == L.OK
    try:
        ptrs5, lens5, keep5 = L.blob_args(mixed[0][:5])
        rc = lib.kzg_commit_and_prove_blob_batch(ctx.handle, tau_srs.handle, ptrs5, lens5, 5, L.ptr(out), None, L.ptr(out), None, None, None, C.byref(bad))
        assert rc == L.ERR_INVALID_ARG
        assert lib.kzg_compute_proof_batch(ctx.handle, tau_srs.handle, L.ptr(ev), 64, 2, L.ptr(z2), L.ptr(out), None, None) == L.ERR_INVALID_ARG
    finally:
        res = np.zeros(8, dtype=np.uint64); inf = C.c_uint8(0)
        assert lib.kzg_msm_g1_srs_end(ctx.handle, 1, L.ptr(res), C.byref(inf), None) == L.OK
    assert np.array_equal(res, mixed[1][3][0])
    com2, proofs2, _, _ = kzg.commit_and_prove_blob_batch(mixed[0][:5], tau_srs)
    for j in range(5):
        assert np.array_equal(com2[j], mixed[1][j][0]) and np.array_equal(proofs2[j], mixed[1][j][1]), j


# ---- the bound-checked build runs the comparisons with every site counter at 0 ------------------------------------------------------------------
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
WORKLOAD = ["tests/test_gpu_prove_batch.py::" + t for t in ("test_golden_rows_in_one_call", "test_every_size_equals_single_calls_and_oracle",
                                                            "test_mixed_lengths_in_one_bytes_call")]


def test_bound_checked_build_keeps_every_precondition():
    """The device build with the lazy-reduction preconditions of csrc/field29.h counted (`make boundcheck`): the golden rows, every size with its
    points on the domain and the mixed blobs, then every site counter of every unit must be 0."""
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": WORKLOAD}], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "PYTEST_RC 0" in out, (out[-3000:], res.stderr[-2000:])
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert sites
    fired = {int(s[1]): int(s[2]) for s in sites if int(s[2])}
    assert not fired, fired
