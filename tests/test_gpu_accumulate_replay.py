"""-m gpu: k_msm_accumulate adds with the UNCHECKED mixed addition and detects P == +-Q once per finished partial sum (ZZ == 0 mod p),
then recomputes that partial with the checked addition (csrc/msm_kernels.h acc_replay).  These commitments make that path run.

All of them are MSMs in NAF table mode (SRS of 2^14 .. 2^16 points: per-bit tables; >= 2^14 pairs: k_msm_accumulate, not the fused
level) over UPLOADED point sets whose rows repeat a point or its negative, with equal scalars on the repeated rows: equal scalars have
equal digits, so the copies meet in one bucket.  Every point is a small multiple s_j G of the generator, so the expected value is
(sum_j c_j s_j) G by big integers (tests/pyref.py), compared bit for bit.

  all equal, uniform scalars   every row is G.  A partial of two or more entries starts G + G (doubling) and goes on with + G: an
                               exceptional pair FOLLOWED BY further entries.  At 2^16 pairs a lane holds ~5-8 entries and a bucket ~64:
                               first partials of a lane, parked partials (a bucket ends inside the lane's range), continuation
                               partials and runs of more than RUN_SERIAL lanes (segmented scan) all replay.  At 2^14 pairs a lane
                               holds ~2 entries: lanes that cross two boundaries (the direct store behind an occupied park slot).
  all equal, 3 scalars         few distinct scalars: a few dozen HEAVY buckets of thousands of entries, runs over many waves.
  +-G alternating, pairs       rows G, -G, G, -G .. with c_2j = c_2j+1: G + (-G) inside every bucket; partials of an even number of
                               entries SUM TO INFINITY, odd ones go on from the identity; the whole commitment is the identity.
  +-G alternating, uniform     the same rows, independent scalars: G + G, G - G and ordinary additions mixed.
  doubled rows                 distinct points P_j (powers of tau), row 2j = row 2j+1 = P_j, c_2j = c_2j+1: exceptional pairs among
                               ordinary entries wherever the two copies open a partial (no count asserted: the order inside a bucket
                               is the sort's).
Each set runs WITHOUT an identity row (k_msm_accumulate<false>: the instantiation without the per-entry identity test) and WITH
identity rows (k_msm_accumulate<true>), one at a time and with TWO MSMs IN FLIGHT (slots 0 and 1).

The hooks build (libkzg_bn254_mi355x_hooks.so, -DKZG_TEST_HOOKS) counts the replays: > 0 on every constructed set, so the test cannot
pass by never taking the new path, and == 0 on the benchmark's own inputs (2^20-point SRS of powers of tau, bench.py's scalars), so
the benchmark pays for none."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import sys
import zlib

import numpy as np
import pytest

import pyref
from pyref import R_

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOOKS = os.path.join(ROOT, "rust-kzg-bn254_amd", "libkzg_bn254_mi355x_hooks.so")
TAU = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % R_
G = (1, 2)

# (name, log2 of the SRS, pairs, replays guaranteed by construction)
CASES = [
    ("all equal, uniform scalars", 16, 1 << 16, True),
    ("all equal, uniform scalars", 14, 1 << 14, True),
    ("all equal, 3 scalars", 15, 1 << 15, True),
    ("+-G alternating, pairs", 16, 1 << 16, True),
    ("+-G alternating, uniform", 15, (1 << 14) + 2, True),
    ("doubled rows", 15, 1 << 15, False),
]
IDS = ["%s 2^%d n=%d" % (c[0], c[1], c[2]) for c in CASES]


def scalars_to_wire(vals):
    mont = (1 << 256) % R_
    return np.frombuffer(b"".join((v * mont % R_).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def build_case(k, name, log_srs, n, with_identity):
    """-> (wire points of the SRS, s: row j is s_j G (None: not a multiple we track), two scalar sets, their expected points)"""
    N = 1 << log_srs
    rnd = random.Random(zlib.crc32(repr((name, log_srs, n, with_identity)).encode()))
    if name == "doubled rows":
        base = k.SRS.generate(TAU, N // 2)
        half = base.g1.reshape(-1, 8)
        base.close()
        pts = np.repeat(half, 2, axis=0).copy()
        s = [pow(TAU, j // 2, R_) for j in range(N)]
    else:
        s = [1] * N if name.startswith("all equal") else [1 if j % 2 == 0 else R_ - 1 for j in range(N)]
        pts = None
    if with_identity:
        for j in (0, 5, N // 2 + 1, n - 1):
            s[j] = 0
    if pts is None:
        wire = {v: pyref.point_to_wire(pyref.ec_mul(v, G) if v else None) for v in set(s)}
        pts = np.stack([wire[v] for v in s])
    else:
        for j in range(N):
            if s[j] == 0:
                pts[j] = 0
    sets = []
    for _ in range(2):
        if name.endswith("3 scalars"):
            three = [rnd.randrange(R_) for _ in range(3)]
            c = [three[rnd.randrange(3)] for _ in range(n)]
        elif name.endswith("pairs") or name == "doubled rows":
            half_c = [rnd.randrange(R_) for _ in range((n + 1) // 2)]
            c = [half_c[j // 2] for j in range(n)]
        else:
            c = [rnd.randrange(R_) for _ in range(n)]
        sets.append(c)
    want = [pyref.ec_mul(sum(a * b for a, b in zip(c, s)) % R_, G) for c in sets]
    return pts, sets, want


def run_case(k, case, with_identity, replays=None):
    """One point set: each scalar set alone, then both in flight.  replays: callable -> replays since the last call (hooks build)."""
    name, log_srs, n, guaranteed = case
    lib = k._lib.load()
    ctx = k.default_context()
    pts, sets, want = build_case(k, name, log_srs, n, with_identity)
    if name.endswith("pairs") and not with_identity:
        assert want[0] is None and want[1] is None                      # every pair cancels
    srs = k.SRS(pts)
    try:
        assert lib.kzg_srs_has_bit_tables(srs.handle, 0) == 1, "no per-bit tables: not the NAF mode"
        wires = [scalars_to_wire(c) for c in sets]
        if replays:
            replays()
        for c_wire, w in zip(wires, want):
            out = np.zeros(8, np.uint64); inf = C.c_uint8(0)
            assert lib.kzg_msm_g1_srs(ctx.handle, srs.handle, 0, k._lib.ptr(c_wire), n, k._lib.ptr(out), C.byref(inf)) == 0
            assert pyref.point_from_wire(out) == w, (name, log_srs, n, with_identity)
            assert bool(inf.value) == (w is None)
        if replays:
            r = replays()
            print("REPLAYS %r identity=%s one at a time: %d" % (IDS[CASES.index(case)], with_identity, r))
            assert r > 0 or not guaranteed, (name, log_srs, n, with_identity, "the replay path never ran")
        outs = [np.zeros(8, np.uint64) for _ in range(2)]
        infs = [C.c_uint8(0) for _ in range(2)]
        for slot in range(2):
            assert lib.kzg_msm_g1_srs_begin(ctx.handle, srs.handle, 0, k._lib.ptr(wires[slot]), n, slot) == 0
        for slot in range(2):
            assert lib.kzg_msm_g1_srs_end(ctx.handle, slot, k._lib.ptr(outs[slot]), C.byref(infs[slot]), None) == 0
        for slot in range(2):
            assert pyref.point_from_wire(outs[slot]) == want[slot], (name, log_srs, n, with_identity, "two in flight", slot)
            assert bool(infs[slot].value) == (want[slot] is None)
        if replays:
            r = replays()
            print("REPLAYS %r identity=%s two in flight: %d" % (IDS[CASES.index(case)], with_identity, r))
            assert r > 0 or not guaranteed, (name, log_srs, n, with_identity, "two in flight: the replay path never ran")
    finally:
        srs.close()


def bench_inputs_replays(k, replays):
    """The benchmark's own commitment (bench.py: 2^20 powers of tau, its first scalar set): the expected point, and no replay."""
    sys.path.insert(0, ROOT)
    import bench
    n = 1 << bench.LOG_N
    lib = k._lib.load()
    ctx = k.default_context()
    canon = bench.blob_like_canonical(n, 0x4B5A472D424E3235 & 0x7FFFFFFF)
    wire = bench.ints_to_wire(canon)
    srs = k.SRS.generate(TAU, n)
    try:
        replays()
        out = np.zeros(8, np.uint64); inf = C.c_uint8(0)
        for _ in range(3):
            assert lib.kzg_msm_g1_srs(ctx.handle, srs.handle, 0, k._lib.ptr(wire), n, k._lib.ptr(out), C.byref(inf)) == 0
        assert np.array_equal(out, bench.expected_commitment(canon, TAU))
        r = replays()
        print("REPLAYS bench inputs 2^%d: %d" % (bench.LOG_N, r))
        assert r == 0, "the benchmark's inputs recompute %d partial sums" % r
    finally:
        srs.close()


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


@pytest.mark.parametrize("with_identity", [False, True], ids=["no identity row", "identity rows"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_commitments_over_repeated_and_opposite_rows(k, case, with_identity):
    """The shipped library: bit-exact values on every set."""
    run_case(k, case, with_identity)


CHILD = r'''
import ctypes as C, os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import torch  # noqa: F401  (load order: tests/conftest.py)
import rust_kzg_bn254_amd as k
L = [m for name, m in list(sys.modules.items()) if name.endswith("_lib") and hasattr(m, "LIB_PATH")][0]
assert L.LIB_PATH == os.environ["KZG_LIB_PATH"], L.LIB_PATH
k.load()
k.default_context()
h = C.CDLL(L.LIB_PATH)
h.kzg_test_acc_replays.restype = C.c_int
h.kzg_test_acc_replays.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
def replays():
    v = C.c_ulonglong(0)
    assert h.kzg_test_acc_replays(C.byref(v), 1) == 0
    return int(v.value)
import test_gpu_accumulate_replay as t
for case in t.CASES:
    for with_identity in (False, True):
        t.run_case(k, case, with_identity, replays)
t.bench_inputs_replays(k, replays)
print("REPLAY_CHILD_OK")
'''


def test_replays_are_counted_on_these_sets_and_absent_on_the_bench_inputs():
    """The hooks build in a fresh process: the same sets with the replay counter > 0 after each, and 0 replays on bench.py's inputs."""
    assert os.path.exists(HOOKS), "make -C rust-kzg-bn254_amd/csrc hooks (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=HOOKS)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    print("\n".join(ln for ln in res.stdout.splitlines() if ln.startswith("REPLAYS")))
    assert res.returncode == 0 and "REPLAY_CHILD_OK" in res.stdout, (res.stdout[-3000:], res.stderr[-3000:])
