"""-m gpu: the G2 kernels with the lazy-reduction preconditions of csrc/field29.h checked on the device.  A fresh child process loads
libkzg_bn254_mi355x_boundcheck.so (the product compiled with -DKZG_DEVICE_BOUND_CHECK) through KZG_LIB_PATH, resets the per-site
counters, runs tests/test_gpu_g2_msm.py and the 2^12 known-tau commitments of tests/test_gpu_g2_srs.py -- every fq2 / curve_g2 formula
on random, edge and degenerate inputs -- and then every counter must be 0, as tests/test_gpu_bound_checked_kernels.py does for G1."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VARIANT = os.path.join(ROOT, "rust-kzg-bn254_amd", "libkzg_bn254_mi355x_boundcheck.so")

WORKLOAD = ["tests/test_gpu_g2_msm.py", "tests/test_gpu_g2_srs.py::test_known_tau_commitments_coefficient_and_evaluation_form[12]",
            "tests/test_gpu_g2_srs.py::test_generate_against_the_fixed_base_multiplication[65-12345]"]
N_SITES = 14

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


def test_g2_kernels_stay_inside_every_precondition():
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
