"""-m gpu: the per-lane G2 chains (csrc/g2_chain.h, g2batch.hip) with the lazy-reduction preconditions of csrc/field29.h checked on the
device.  A fresh child process loads libkzg_bn254_mi355x_boundcheck.so (the product compiled with -DKZG_DEVICE_BOUND_CHECK) through
KZG_LIB_PATH, resets the per-site counters, verifies one honest batch of 65 headers in three groups -- the subgroup chain, the
128-bit weighted chains, the shuffle tree -- and then every counter must be 0, as tests/test_gpu_g2_bound_checked.py does for the MSM."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VARIANT = os.path.join(ROOT, "rust-kzg-bn254_amd", "libkzg_bn254_mi355x_boundcheck.so")
N_SITES = 14

CHILD = r'''
import ctypes as C, os, random, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import torch  # noqa: F401  (load order: tests/conftest.py)
import numpy as np
import rust_kzg_bn254_amd as k
import pyref
from pyref import R_
L = k._lib
assert L.LIB_PATH == os.environ["KZG_LIB_PATH"], L.LIB_PATH
h = L.load()
n = h.kzg_bc_sites()
assert n == %(sites)d, n
assert h.kzg_bc_reset_all() == 0
rnd = random.Random(5)
N, tau = 1024, rnd.randrange(2, R_)
g1 = lambda s: pyref.point_to_wire(pyref.ec_mul(s %% R_, (1, 2)))
g2 = lambda s: k.helpers.g2_mul_generator(pyref.fr_to_mont(s %% R_))
lens = [1 if i %% 2 else 4 for i in range(65)]
lens[32] = 1024
fs = [rnd.randrange(1, R_) for _ in lens]
shifts = {d: g1(pow(tau, N - d, R_)) for d in (1, 4, 1024)}
c = np.stack([g1(f) for f in fs]); c2 = np.stack([g2(f) for f in fs])
pi2 = np.stack([g2(pow(tau, N - d, R_) * f) for f, d in zip(fs, lens)])
ok = k.verifier.verify_length_proof_batch(c, c2, pi2, lens, shifts)
full = pyref.frs_to_mont([rnd.randrange(R_) for _ in range(66)])            # 254-bit chains
ok2 = k.verifier.verify_length_proof_batch(c, c2, pi2, lens, shifts, weights=full)
counts = (C.c_ulonglong * n)(); first = (C.c_int32 * (9 * n))()
assert h.kzg_bc_read_all(counts, first) == 0
print("ACCEPTED", int(ok), int(ok2))
for s in range(n):
    print("SITE", s, counts[s], *first[9 * s:9 * s + 9])
'''


def test_header_batch_kernels_stay_inside_every_precondition():
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    body = CHILD % {"root": ROOT, "sites": N_SITES}
    res = subprocess.run([sys.executable, "-c", body], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "ACCEPTED 1 1" in out, (out[-3000:], res.stderr[-2000:])
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert len(sites) == N_SITES
    fired = [(int(s[1]), int(s[2]), s[3:]) for s in sites if int(s[2]) != 0]
    assert not fired, "bound violations on the device (site, count, first operand limbs): %r" % (fired,)
