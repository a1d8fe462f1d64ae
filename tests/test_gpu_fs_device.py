"""-m gpu: Fiat-Shamir hashing on the device (csrc/dev_sha256.h, csrc/coset_item_stream.h, csrc/fsdevice.hip): `kzg_sha256_rows` against
hashlib at the padding boundaries and the wave / workgroup edges; `kzg_compute_multiproof_r_powers_device` bit-equal to the host entry
and to the Python transcript, with the host fallback for inputs that are not canonical; `kzg_verify_multiproof_batch` on a 64-point
domain with the transcript forced onto the device and onto the host (`Context.set_transcript_device`).  Every comparison is exact."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pyref
from pyref import P, R_

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROW_LENS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 2120]
TAU = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/fs-device/v1").digest(), "big") % R_
N = 64


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


def words(value):
    return [(value >> (64 * j)) & (2**64 - 1) for j in range(4)]


# ---- 1. the primitive -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_sha256_rows_against_hashlib(k, count):
    """one lane per row, one wave per workgroup: 63 / 64 / 65 rows end a wave, fill it, open the next; 257 rows are five workgroups"""
    rng = np.random.default_rng(count)
    for row_len in ROW_LENS:
        rows = rng.integers(0, 256, (count, row_len), dtype=np.uint8)
        got = k.helpers.sha256_rows(rows)
        assert got.shape == (count, 32) and got.dtype == np.uint8
        for i in range(count):
            assert got[i].tobytes() == hashlib.sha256(rows[i].tobytes()).digest(), (count, row_len, i)


def test_sha256_rows_degenerate_shapes_and_errors(k):
    L = k._lib
    lib, ctx = L.load(), k.default_context()
    assert k.helpers.sha256_rows(np.zeros((0, 7), np.uint8)).shape == (0, 32)
    empty = k.helpers.sha256_rows(np.zeros((3, 0), np.uint8))
    assert all(row.tobytes() == hashlib.sha256(b"").digest() for row in empty)
    out = np.zeros(32, np.uint8)
    msg = np.zeros(8, np.uint8)
    u8 = lambda a: a.ctypes.data_as(L.u8p)                                     # noqa: E731
    assert lib.kzg_sha256_rows(None, u8(msg), 8, 1, u8(out)) == L.ERR_INVALID_ARG
    assert lib.kzg_sha256_rows(ctx.handle, None, 8, 1, u8(out)) == L.ERR_INVALID_ARG
    assert lib.kzg_sha256_rows(ctx.handle, u8(msg), 8, 1, None) == L.ERR_INVALID_ARG
    assert lib.kzg_sha256_rows(ctx.handle, u8(msg), 8, (1 << 28) + 1, u8(out)) == L.ERR_TOO_LARGE
    assert lib.kzg_sha256_rows(ctx.handle, u8(msg), (1 << 31) // 2 + 1, 2, u8(out)) == L.ERR_TOO_LARGE
    assert lib.kzg_sha256_rows(ctx.handle, None, 0, 0, None) == L.OK
    with pytest.raises(ValueError):
        ctx.set_transcript_device(3)


# ---- 2. the weights ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def points():
    """wire points: the identity, a point whose y is the larger root, its negative, two more"""
    rnd = random.Random(21)
    pts = []
    while len(pts) < 2:
        pt = pyref.ec_mul(rnd.randrange(1, R_), (1, 2))
        if not pts and pt[1] <= (P - 1) // 2:
            continue
        pts.append(pt)
    big = pts[0]
    return [np.zeros(8, np.uint64), pyref.point_to_wire(big), pyref.point_to_wire((big[0], P - big[1])), pyref.point_to_wire(pts[1]),
            pyref.point_to_wire((1, 2))]


def transcript_case(points, l, count, seed):
    rnd = random.Random(seed)
    special = [0, 1, R_ - 1]
    y_int = [[rnd.choice(special) if rnd.random() < 0.1 else rnd.randrange(R_) for _ in range(l)] for _ in range(count)]
    y_int[0][0], y_int[-1][l - 1], y_int[count // 2][l // 2] = 0, R_ - 1, 1
    ys = np.ascontiguousarray(np.stack([pyref.frs_to_mont(v) for v in y_int]))
    proofs = [points[i % 3] if i < 6 else points[rnd.randrange(len(points))] for i in range(count)]
    commitments = [points[3], points[1]]                                       # two commitments, rows 1 and 0 both used
    rows = [1 - (i % 2) if i < 4 else rnd.randrange(2) for i in range(count)]
    ks = [rnd.randrange(1 << 20) for _ in range(count)]
    return commitments, rows, ks, ys, proofs


@pytest.mark.parametrize("l,count", [(l, c) for l in (1, 2, 16, 64) for c in (1, 65, 300)] + [(1, 4097)])
def test_r_powers_device_is_bit_equal_to_host_and_python(k, points, l, count):
    """(1, 4097): power tables of 128 x 33 entries, lanes on either side of every table row; 65 / 300: a second wave, several workgroups"""
    V = k.verifier
    n = 1 << 24
    args = transcript_case(points, l, count, 31 * l + count)
    dev = V.compute_multiproof_r_powers(*args, n, device=True)
    host = V.compute_multiproof_r_powers(*args, n)
    assert dev.shape == (count, 4) and dev.dtype == np.uint64
    assert np.array_equal(dev, host)
    assert np.array_equal(dev, V.compute_multiproof_r_powers_py(*args, n))
    assert pyref.fr_from_mont(dev[0]) == 1


def test_r_powers_device_power_tables_at_their_edges(k, points):
    """counts on both sides of a square (255, 256, 257: the low table grows from 16 to 32 entries) and of a table row"""
    V = k.verifier
    for count in (2, 3, 4, 5, 255, 256, 257):
        args = transcript_case(points, 1, count, 700 + count)
        assert np.array_equal(V.compute_multiproof_r_powers(*args, 64, device=True), V.compute_multiproof_r_powers(*args, 64)), count


@pytest.mark.parametrize("what", ["value", "coordinate"])
def test_non_canonical_inputs_take_the_host_transcript(k, points, what):
    """a value >= r / a coordinate >= p: the device entry returns exactly what the host entry returns"""
    V = k.verifier
    commitments, rows, ks, ys, proofs = transcript_case(points, 16, 70, 88)
    ys, proofs = ys.copy(), [p.copy() for p in proofs]
    if what == "value":
        ys[66, 15] = words(R_ + 5)
    else:
        proofs[65][4:8] = words(P)
    host = V.compute_multiproof_r_powers(commitments, rows, ks, ys, proofs, 4096)
    dev = V.compute_multiproof_r_powers(commitments, rows, ks, ys, proofs, 4096, device=True)
    assert np.array_equal(dev, host)
    clean = transcript_case(points, 16, 70, 88)
    assert not np.array_equal(V.compute_multiproof_r_powers(*clean, 4096, device=True), host)      # (the input did change the transcript)


def test_r_powers_device_errors_as_the_host_entry(k, points):
    L = k._lib
    lib, ctx = L.load(), k.default_context()
    commitments, rows, ks, ys, proofs = transcript_case(points, 2, 3, 5)
    cm, pf = np.ascontiguousarray(np.stack(commitments)), np.ascontiguousarray(np.stack(proofs))
    ci, ki = np.array(rows, np.uint64), np.array(ks, np.uint64)
    out = np.zeros((3, 4), np.uint64)
    Pn = lambda a: None if a is None else L.ptr(a)                              # noqa: E731

    def call(ctx_h=ctx.handle, cm_=cm, ci_=ci, ki_=ki, ys_=ys, pf_=pf, count=3, l=2, out_=out):
        return lib.kzg_compute_multiproof_r_powers_device(ctx_h, Pn(cm_), 2, Pn(ci_), Pn(ki_), Pn(ys_), Pn(pf_), count, 64, l, Pn(out_))

    assert call() == L.OK
    for kw in (dict(ctx_h=None), dict(cm_=None), dict(ci_=None), dict(ki_=None), dict(ys_=None), dict(pf_=None), dict(out_=None), dict(l=0)):
        assert call(**kw) == L.ERR_INVALID_ARG, kw
    assert call(count=(1 << 28) // 2 + 1) == L.ERR_TOO_LARGE
    assert call(count=0, ys_=None) == L.OK


# ---- 3. the batch verifier with the transcript on either side ------------------------------------------------------------------
class World:
    """Two random polynomials of 64 evaluations on a known-tau SRS; per chunk length their proofs, cosets and [tau^l]_2."""

    def __init__(self, k):
        self.k = k
        self.ctx = k.default_context()
        self.srs = k.SRS.generate(TAU, N)
        self.kz = k.KZG.new()
        self.kz.calculate_and_store_roots_of_unity(N * 32)
        rnd = random.Random(64)
        self.polys = [k.PolynomialEvalForm(pyref.frs_to_mont([rnd.randrange(R_) for _ in range(N)])) for _ in range(2)]
        self.commitments = [self.kz.commit_eval_form(p, self.srs) for p in self.polys]
        self._by_l = {}

    def at(self, l):
        if l not in self._by_l:
            self._by_l[l] = ([self.kz.compute_multiproofs(p, self.srs, l) for p in self.polys], [self.kz.cosets(p, l) for p in self.polys],
                             self.k.helpers.g2_mul_generator(self.k.fr.fr_from_int(pow(TAU, l, R_))))
        return self._by_l[l]

    def items(self, l, rows, ks):
        proofs, cosets, g2 = self.at(l)
        return np.ascontiguousarray(np.stack([cosets[c][kk] for c, kk in zip(rows, ks)])), [proofs[c][kk] for c, kk in zip(rows, ks)], g2

    def verify(self, rows, ks, ys, pf, g2, r_powers=None):
        return self.k.verifier.verify_multiproof_batch(self.commitments, rows, ks, ys, pf, N, self.srs, g2, r_powers)


@pytest.fixture(scope="module")
def world(k):
    return World(k)


@pytest.fixture(params=[2, 1], ids=["device", "host"])
def mode(request, world):
    world.ctx.set_transcript_device(request.param)
    yield request.param
    world.ctx.set_transcript_device(0)


@pytest.mark.parametrize("l", [1, 4, 16])
def test_verify_multiproof_batch_with_the_transcript_on_either_side(k, world, mode, l):
    """every proof of compute_multiproofs accepted; one corrupted value, proof or coset index rejected; a duplicated item accepted; the
    empty batch accepted; supplied weights give the same answers"""
    m = N // l
    rows = [c for c in range(2) for _ in range(m)]
    ks = list(range(m)) * 2
    ys, pf, g2 = world.items(l, rows, ks)
    rp = k.verifier.compute_multiproof_r_powers(world.commitments, rows, ks, ys, pf, N)

    def both(rows_, ks_, ys_, pf_, rp_):
        a, b = world.verify(rows_, ks_, ys_, pf_, g2), world.verify(rows_, ks_, ys_, pf_, g2, r_powers=rp_)
        assert a is b
        return a

    assert both(rows, ks, ys, pf, rp) is True
    bad = ys.copy()
    bad[m + 1, l - 1] = k.fr.fr_from_int(k.fr.fr_to_int(bad[m + 1, l - 1]) + 1)
    assert both(rows, ks, bad, pf, rp) is False                                # one value off by one
    swapped = list(pf)
    swapped[0], swapped[1] = swapped[1], swapped[0]
    assert both(rows, ks, ys, swapped, rp) is False                            # the proofs of two cosets swapped
    ks2 = list(ks)
    ks2[2] = (ks2[2] + 1) % m
    assert both(rows, ks2, ys, pf, rp) is False                                # a coset index off by one
    rows3, ks3 = rows + [rows[5 % len(rows)]], ks + [ks[5 % len(ks)]]
    ys3, pf3, _ = world.items(l, rows3, ks3)
    assert both(rows3, ks3, ys3, pf3, k.verifier.compute_multiproof_r_powers(world.commitments, rows3, ks3, ys3, pf3, N)) is True   # a duplicated item
    assert world.verify([], [], np.zeros((0, l, 4), np.uint64), [], g2) is True
    assert both(rows, ks, ys, pf, rp) is True


def test_error_codes_in_the_documented_order_on_either_side(k, world, mode):
    L = k._lib
    lib = L.load()
    l, m = 4, N // 4
    rows, ks = [0, 1, 1], [3, 0, m - 1]
    ys, pf, g2 = world.items(l, rows, ks)
    cm, pf = np.ascontiguousarray(np.stack(world.commitments)), np.ascontiguousarray(np.stack(pf))
    ci, ki = np.array(rows, np.uint64), np.array(ks, np.uint64)
    ok = L.i32(7)
    Pn = lambda a: None if a is None else L.ptr(a)                              # noqa: E731

    def call(ys_=ys, ki_=ki, pf_=pf, n_=N, g2_=g2):
        return lib.kzg_verify_multiproof_batch(world.ctx.handle, world.srs.handle, Pn(cm), 2, Pn(ci), Pn(ki_), Pn(ys_), Pn(pf_), 3, n_, l, None, Pn(g2_), C.byref(ok))

    assert call() == L.OK and ok.value == 1
    ok.value = 7
    off, bad_g2 = pf.copy(), g2.copy()
    off[1, 4] ^= 1
    bad_g2[0] ^= 1
    assert call(ys_=None) == L.ERR_INVALID_ARG
    assert call(n_=96) == L.ERR_NOT_POWER_OF_TWO
    assert call(n_=96, ki_=np.array([3, 0, m], np.uint64)) == L.ERR_NOT_POWER_OF_TWO       # the domain before the indices
    assert call(ki_=np.array([3, 0, m], np.uint64)) == L.ERR_INVALID_ARG
    assert call(ki_=np.array([3, 0, m], np.uint64), pf_=off) == L.ERR_INVALID_ARG          # the indices before the points
    assert call(pf_=off) == L.ERR_G1_NOT_ON_CURVE
    assert call(pf_=off, g2_=bad_g2) == L.ERR_G1_NOT_ON_CURVE                              # a bad G1 point before a bad G2 point
    assert call(g2_=bad_g2) == L.ERR_G2_TAU_NOT_ON_CURVE
    assert ok.value == 7                                                       # no error path writes the verdict
    assert call() == L.OK and ok.value == 1


def test_non_canonical_value_in_a_batch_gives_the_same_verdict_on_either_side(k, world):
    """the device path detects the value, recomputes the transcript on the host and goes on.  y + r is the residue y, so the batch still holds
    (the interpolation reads wire words below 2^256 as they are) and both sides accept; one more off-by-one value and both reject"""
    l, m = 4, N // 4
    rows, ks = [0] * m, list(range(m))
    ys, pf, g2 = world.items(l, rows, ks)
    ys = ys.copy()
    ys[3, 2] = words(pyref.from_limbs(ys[3, 2]) + R_)                           # the same residue, not canonical
    verdicts = []
    try:
        for md in (1, 2):
            world.ctx.set_transcript_device(md)
            verdicts.append(world.verify(rows, ks, ys, pf, g2))
        wrong = ys.copy()
        wrong[5, 0] = k.fr.fr_from_int(k.fr.fr_to_int(wrong[5, 0]) + 1)
        for md in (1, 2):
            world.ctx.set_transcript_device(md)
            verdicts.append(world.verify(rows, ks, wrong, pf, g2))
    finally:
        world.ctx.set_transcript_device(0)
    assert verdicts == [True, True, False, False]


# ---- 4. the bound-checked build runs the weights and the forced-device verifier with every site counter at 0 ---------------------
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
WORKLOAD = ["tests/test_gpu_fs_device.py::" + t for t in (
    "test_r_powers_device_is_bit_equal_to_host_and_python", "test_r_powers_device_power_tables_at_their_edges",
    "test_non_canonical_inputs_take_the_host_transcript", "test_verify_multiproof_batch_with_the_transcript_on_either_side")]


def test_bound_checked_build_keeps_every_precondition():
    """the Montgomery -> canonical conversions of the item stream and the product of k_fr_powers under -DKZG_DEVICE_BOUND_CHECK (inputs at
    and above the modulus included): no lazy-reduction precondition is violated"""
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": WORKLOAD}], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "PYTEST_RC 0" in out, (out[-3000:], res.stderr[-2000:])
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert sites
    fired = {int(s[1]): int(s[2]) for s in sites if int(s[2])}
    assert not fired, fired
