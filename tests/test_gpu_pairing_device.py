"""-m gpu: batches of pairing checks on the device (`kzg_pairings_product_verify_batch`, `kzg_pairings_product_gt_batch`; csrc/pairing.hip).

Truth is the host: `kzg_pairings_product_gt` for every value, bit for bit, and `verifier.pairings_product_verify` for every verdict.  The
batches mix checks of 0, 1, 2, 3, 4 and 5 pairs (5 crosses the shared loop's four), true relations and spoiled ones, at 1, 63, 64, 65 and
130 checks (a wave of 64 lanes, its neighbours, more than two waves).  A true relation is built from blocks sum_i e(P_i, Q) e(-sum P_i, Q)
over multiples of the generators with known scalars; a spoiled one has one G1 point replaced.

The parity tests also run in a child process under libkzg_bn254_mi355x_boundcheck.so (the lazy-reduction preconditions of csrc/field29.h
counted on the device, as tests/test_gpu_g2_bound_checked.py does for the G2 kernels): 14 sites, every counter 0."""
import ctypes as C
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

import g2_points as g2
import pyref
from pyref import R_

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VARIANT = os.path.join(ROOT, "rust-kzg-bn254_amd", "libkzg_bn254_mi355x_boundcheck.so")
N_SITES = 14
Z1, Z2 = np.zeros(8, np.uint64), np.zeros(16, np.uint64)


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


class Pool:
    """multiples of the two generators with their scalars: 40 in G1 (as integer points too, for the sums), 12 in G2"""

    def __init__(self, k):
        rnd = random.Random(197)
        self.a = [rnd.randrange(1, R_) for _ in range(40)]
        self.p = [pyref.ec_mul(a, (1, 2)) for a in self.a]
        self.q = [k.helpers.g2_mul_generator(pyref.fr_to_mont(rnd.randrange(1, R_))) for _ in range(12)]

    def block(self, rnd, size):
        """`size` pairs (2 or 3) whose product is one: e(P1, Q) [e(P2, Q)] e(-(P1 [+ P2]), Q)"""
        q = self.q[rnd.randrange(len(self.q))]
        ps = [self.p[rnd.randrange(len(self.p))] for _ in range(size - 1)]
        total = None
        for p in ps:
            total = pyref.ec_add(total, p)
        g1s = [pyref.point_to_wire(p) for p in ps] + [pyref.point_to_wire(pyref.ec_neg(total) if total is not None else None)]
        order = list(range(size))
        rnd.shuffle(order)
        return [g1s[i] for i in order], [q] * size

    def check(self, rnd, pairs, spoil):
        """(g1s, g2s) of one check of `pairs` pairs; true unless spoil (or pairs == 1: a lone pair of two non-identity points is never one)"""
        if pairs == 0:
            return [], []
        if pairs == 1:
            return [pyref.point_to_wire(self.p[rnd.randrange(len(self.p))])], [self.q[rnd.randrange(len(self.q))]]
        sizes = {2: [2], 3: [3], 4: [2, 2], 5: [2, 3]}[pairs]
        g1s, g2s = [], []
        for s in sizes:
            a, b = self.block(rnd, s)
            g1s += a; g2s += b
        if spoil:
            g1s[rnd.randrange(pairs)] = pyref.point_to_wire(pyref.ec_mul(rnd.randrange(1, R_), (1, 2)))
        return g1s, g2s


@pytest.fixture(scope="module")
def pool(k):
    return Pool(k)


def _batch(checks):
    off = np.cumsum([0] + [len(c[0]) for c in checks]).astype(np.uint64)
    g1s = np.stack([p for c in checks for p in c[0]] or [Z1])[:int(off[-1])].reshape(-1, 8)
    g2s = np.stack([q for c in checks for q in c[1]] or [Z2])[:int(off[-1])].reshape(-1, 16)
    return g1s, g2s, off


def _host(k, checks):
    gt = np.stack([k.verifier.pairings_product_gt(np.array(c[0], np.uint64).reshape(-1, 8), np.array(c[1], np.uint64).reshape(-1, 16)) for c in checks])
    ok = np.array([k.verifier.pairings_product_verify(np.array(c[0], np.uint64).reshape(-1, 8), np.array(c[1], np.uint64).reshape(-1, 16)) for c in checks])
    return gt, ok


def _compare(k, checks):
    g1s, g2s, off = _batch(checks)
    want_gt, want_ok = _host(k, checks)
    got_gt = k.verifier.pairings_product_gt_batch(g1s, g2s, off)
    got_ok = k.verifier.pairings_product_verify_batch(g1s, g2s, off)
    assert got_gt.shape == want_gt.shape and got_ok.shape == want_ok.shape
    differ = [i for i in range(len(checks)) if not np.array_equal(got_gt[i], want_gt[i])]
    assert not differ, "GT values differ from the host's at checks %r" % differ[:8]
    assert np.array_equal(got_ok, want_ok), np.nonzero(got_ok != want_ok)[0][:8]
    return want_ok


@pytest.mark.parametrize("n_checks", [1, 63, 64, 65, 130])
def test_values_and_verdicts_equal_the_host(k, pool, n_checks):
    rnd = random.Random(1000 + n_checks)
    first = 2 if n_checks == 1 else n_checks % 6                    # where the cycle 0, 1, .., 5 of pair counts starts
    checks = [pool.check(rnd, (first + i) % 6, spoil=(i % 3 == 1)) for i in range(n_checks)]
    ok = _compare(k, checks)
    if n_checks > 6:
        assert ok.any() and not ok.all()
        for i, c in enumerate(checks):                              # what was built: an empty or unspoiled check of blocks holds, every other one fails
            assert bool(ok[i]) == (len(c[0]) == 0 or (len(c[0]) > 1 and i % 3 != 1)), i


def test_identity_points_in_the_first_middle_and_last_position(k, pool):
    rnd = random.Random(5)
    checks = []
    for pos in (0, 1, 2):
        for which in (0, 1, 2):                                     # an identity in G1, in G2, in both
            a, b = pool.check(rnd, 2, spoil=False)
            other = pool.check(rnd, 1, spoil=False)                 # the partner of the identity: any point
            a.insert(pos, Z1 if which != 1 else other[0][0])
            b.insert(pos, Z2 if which != 0 else other[1][0])
            checks.append((a, b))
    a, b = pool.check(rnd, 5, spoil=False)                          # an identity behind a full chunk of four
    checks.append((a[:4] + [Z1] + a[4:], b[:4] + [b[0]] + b[4:]))
    checks.append(([Z1, Z1], [Z2, pool.q[0]]))                      # nothing but identities
    ok = _compare(k, checks)
    assert ok.all()


@pytest.mark.parametrize("n_checks", [130])
def test_one_false_check_clears_exactly_its_byte(k, pool, n_checks):
    rnd = random.Random(77)
    good = [pool.check(rnd, 2, spoil=False) for _ in range(n_checks)]
    for pos in (0, 63, 64, n_checks - 1):
        checks = list(good)
        checks[pos] = pool.check(rnd, 2, spoil=True)
        g1s, g2s, off = _batch(checks)
        ok = k.verifier.pairings_product_verify_batch(g1s, g2s, off)
        want = np.ones(n_checks, bool)
        want[pos] = False
        assert np.array_equal(ok, want), (pos, np.nonzero(~ok)[0])


def test_points_off_their_curves_g1_first_and_outputs_untouched(k, pool):
    L = k._lib
    lib, ctx = L.load(), L.default_context()
    rnd = random.Random(9)
    checks = [pool.check(rnd, 2 + i % 3, spoil=False) for i in range(9)]
    g1s, g2s, off = _batch(checks)
    n = len(checks)
    bad1, bad2 = g1s.copy(), g2s.copy()
    bad1[17, 0] ^= np.uint64(1); bad1[20, 5] ^= np.uint64(2)        # two G1 points off the curve: the first is named
    bad2[3, 9] ^= np.uint64(4)                                      # a G2 point off the twist in FRONT of them: the G1 error still wins
    for a, b, rc_want, idx in ((bad1, bad2, L.ERR_G1_NOT_ON_CURVE, 17), (g1s, bad2, L.ERR_G2_TAU_NOT_ON_CURVE, 3), (bad1, g2s, L.ERR_G1_NOT_ON_CURVE, 17)):
        ok = np.full(n, 0xA5, np.uint8)
        gt = np.full((n, 12, 4), 0xA5A5A5A5A5A5A5A5, np.uint64)
        bad = C.c_uint64(1 << 40)
        assert lib.kzg_pairings_product_verify_batch(ctx.handle, L.ptr(a), L.ptr(b), L.ptr(off), n, ok.ctypes.data_as(L.u8p), C.byref(bad)) == rc_want
        assert bad.value == idx and (ok == 0xA5).all()
        bad = C.c_uint64(1 << 40)
        assert lib.kzg_pairings_product_gt_batch(ctx.handle, L.ptr(a), L.ptr(b), L.ptr(off), n, L.ptr(gt), C.byref(bad)) == rc_want
        assert bad.value == idx and (gt == 0xA5A5A5A5A5A5A5A5).all()
        assert lib.kzg_pairings_product_verify_batch(ctx.handle, L.ptr(a), L.ptr(b), L.ptr(off), n, ok.ctypes.data_as(L.u8p), None) == rc_want     # a null bad_index
    with pytest.raises(k.errors.NotOnCurveError, match="G1 point 17"):
        k.verifier.pairings_product_verify_batch(bad1, bad2, off)
    with pytest.raises(k.errors.NotOnCurveError, match="G2 point 3"):
        k.verifier.pairings_product_gt_batch(g1s, bad2, off)
    assert k.verifier.pairings_product_verify_batch(g1s, g2s, off).all()                                # the context still works
    assert len(k.verifier.pairings_product_verify_batch(g1s[:0], g2s[:0], [0])) == 0                   # no checks
    assert k.verifier.pairings_product_verify_batch(g1s[:0], g2s[:0], [0, 0, 0]).all()                 # empty checks only


def test_g2_points_on_the_twist_outside_the_subgroup(k, pool):
    """the library checks the twist equation only, as the host entry does: whatever the host computes for such a point, the device computes"""
    rnd = random.Random(23)
    checks = []
    for i in range(6):
        tw = g2.to_wire(g2.random_twist_point(rnd))
        a, b = pool.check(rnd, 2, spoil=False)
        checks.append((a + [pyref.point_to_wire(pool.p[i])], b + [tw]) if i % 2 else ([pyref.point_to_wire(pool.p[i])], [tw]))
    small = g2.to_wire(g2.point_of_order(10069, rnd))
    checks.append(([pyref.point_to_wire(pool.p[7]), pyref.point_to_wire(pool.p[8])], [small, pool.q[1]]))
    _compare(k, checks)


def test_two_host_threads_on_one_context(k, pool):
    rnd = random.Random(31)
    jobs = []
    for t in range(2):
        checks = [pool.check(rnd, 2 + (i + t) % 4, spoil=(i % 4 == t)) for i in range(20 + 50 * t)]
        jobs.append((checks,) + _host(k, checks))
    errors = []

    def run(checks, want_gt, want_ok):
        try:
            g1s, g2s, off = _batch(checks)
            for _ in range(2):
                assert np.array_equal(k.verifier.pairings_product_gt_batch(g1s, g2s, off), want_gt)
                assert np.array_equal(k.verifier.pairings_product_verify_batch(g1s, g2s, off), want_ok)
        except Exception as e:                                       # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=run, args=j) for j in jobs]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


CHILD = r'''
import ctypes as C, os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import torch  # noqa: F401  (load order: tests/conftest.py)
import rust_kzg_bn254_amd  # noqa: F401
L = [m for name, m in list(sys.modules.items()) if name.endswith("_lib") and hasattr(m, "LIB_PATH")][0]
assert L.LIB_PATH == os.environ["KZG_LIB_PATH"], L.LIB_PATH
h = L.load()
n = h.kzg_bc_sites()
assert n == %(sites)d, n
assert h.kzg_bc_reset_all() == 0
import pytest
rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", "-x", *%(tests)r])
counts = (C.c_ulonglong * n)(); first = (C.c_int32 * (9 * n))()
assert h.kzg_bc_read_all(counts, first) == 0
print("PYTEST_RC", int(rc))
for s in range(n):
    print("SITE", s, counts[s], *first[9 * s:9 * s + 9])
'''
WORKLOAD = ["tests/test_gpu_pairing_device.py::test_values_and_verdicts_equal_the_host[65]",
            "tests/test_gpu_pairing_device.py::test_identity_points_in_the_first_middle_and_last_position",
            "tests/test_gpu_pairing_device.py::test_g2_points_on_the_twist_outside_the_subgroup"]


def test_pairing_kernels_stay_inside_every_precondition():
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    body = CHILD % {"root": ROOT, "sites": N_SITES, "tests": WORKLOAD}
    res = subprocess.run([sys.executable, "-c", body], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "PYTEST_RC 0" in out, (out[-3000:], res.stderr[-2000:])
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert len(sites) == N_SITES
    fired = [(int(s[1]), int(s[2]), s[3:]) for s in sites if int(s[2]) != 0]
    assert not fired, "bound violations on the device (site, count, first operand limbs): %r" % (fired,)
