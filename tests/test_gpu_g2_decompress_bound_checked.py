"""-m gpu: the device decoder of compressed G2 points (csrc/g2_decode.h, k_g2_decompress of csrc/g2decode.hip) with the lazy-reduction
preconditions of csrc/field29.h checked on the device.  A fresh child process loads libkzg_bn254_mi355x_boundcheck.so (the product
compiled with -DKZG_DEVICE_BOUND_CHECK) through KZG_LIB_PATH, resets the per-site counters, runs the golden-file, round-trip and error
tests of tests/test_gpu_g2_decompress.py -- both branches of the square root, both flags, coordinates at and above the modulus, points
off the twist and outside the subgroup -- and then every counter must be 0, as tests/test_gpu_g2_bound_checked.py does for the G2 MSM."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VARIANT = os.path.join(ROOT, "rust-kzg-bn254_amd", "libkzg_bn254_mi355x_boundcheck.so")

T = "tests/test_gpu_g2_decompress.py::"
WORKLOAD = [T + "test_golden_file_equals_the_host_decoder_bit_for_bit", T + "test_round_trip_of_300_generated_points_with_both_flags",
            T + "test_errors_equal_the_host_decoder_and_leave_the_context_usable", T + "test_the_smallest_bad_index_is_reported_with_its_own_kind"]
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


def test_g2_decoder_stays_inside_every_precondition():
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
