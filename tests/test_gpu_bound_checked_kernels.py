"""-m gpu: the product's kernels with the lazy-reduction preconditions of csrc/field29.h checked on the device.

libkzg_bn254_mi355x_boundcheck.so (`make boundcheck`, built by __graft_entry__.build()) is the product compiled with
-DKZG_DEVICE_BOUND_CHECK: every fe_mul / fe_sqr / fe_mul2 / fe_sqr2 / fe_mulsub operand pair, every fe_is_zero_mod / fe_canon /
fe_reduce / fe_reduce_small / fe_to_wire / fe_pack input and every fe_add / fe_sub / fe_dbl / fe_norm is tested against the bound its
formula relies on, and a violation counts per site (the first one keeps its operand limbs).  A fresh child process loads the variant
through KZG_LIB_PATH, resets the counters, runs existing GPU tests that compare every output with the oracle or a known tau -- the NTT
at every size and on extreme vectors, every MSM plan (bit sums, table NAF, generic windows 2..16, batched, reduction lanes) on the
adversarial scalar and degenerate point sets, g1_ifft, the Lagrange cache and shards, proofs on and off the domain with every
inversion-chain shape, blob_to_fr, SRS decompression and the device part of batch verification -- and then every counter must be 0.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VARIANT = os.path.join(ROOT, "rust-kzg-bn254_amd", "libkzg_bn254_mi355x_boundcheck.so")

WORKLOAD = [
    "tests/test_gpu_parity.py::" + t for t in (
        "test_ntt_extreme_values", "test_ntt_matches_oracle", "test_msm_edge_cases", "test_msm_adversarial_digit_patterns",
        "test_msm_every_window_size", "test_table_mode_and_generic_mode_agree", "test_tiny_msm_as_sums_of_per_bit_table_points",
        "test_reduction_kernels_on_lane_pairs_and_lane_quads", "test_msm_batch_of_64_small_msms", "test_msm_known_tau_and_oracle",
        "test_g1_ifft_matches_lagrange_fixture_and_oracle", "test_g1_ifft_paths_and_lagrange_cache", "test_proofs_every_inversion_chain_shape",
        "test_proof_off_domain_and_guards", "test_proofs_match_reference_golden_vectors", "test_blob_to_fr_and_commit_blob",
        "test_srs_new_decompresses_reference_file", "test_batched_lincomb_like_batch_verification")
] + [
    "tests/test_gpu_ntt_sizes.py::test_ntt_every_size_matches_oracle",
    "tests/test_gpu_degenerate_points.py",
    "tests/test_gpu_lagrange_shards.py::test_sharded_commit_and_proof_against_the_oracle",
    "tests/test_gpu_verifier.py::test_random_blobs_single_and_batch",
    "tests/test_gpu_verifier.py::test_batched_evaluation_with_points_on_the_domain",
]

SITES = ["mul limbs", "mul value", "fe_mulsub limbs", "fe_mulsub value", "fe_is_zero_mod", "fe_canon", "fe_reduce", "fe_reduce_small",
         "fe_to_wire", "fe_pack", "fe_add", "fe_sub", "fe_dbl", "fe_norm"]

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


def test_kernels_stay_inside_every_precondition():
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    body = CHILD % {"root": ROOT, "sites": len(SITES), "tests": WORKLOAD}
    res = subprocess.run([sys.executable, "-c", body], capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "PYTEST_RC 0" in out, (out[-3000:], res.stderr[-2000:])
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert len(sites) == len(SITES)
    fired = {SITES[int(s[1])]: (int(s[2]), [int(x) for x in s[3:]]) for s in sites if int(s[2])}
    assert not fired, fired
