"""-m gpu: the work-efficient sum tree of the first bucket-reduction level (group_sum_tree, csrc/curve_quad.h; k_msm_bucket_bits1 and
k_msm_bucket_bits1_fused, csrc/msm_kernels.h).

1. The tree on its own: tests/devcheck/treecheck.hip, a stand-alone program, feeds it 64 x {1, 3, 4, 5} points in both lane forms and
   compares slot 0 and the slots 2^k of every group with host sums (inputs: see the head of that file).
2. Through the C-ABI on a known-tau SRS of 2^15 points, every result against (sum_i c_i tau^i) G by big integers (tests/pyref.py), on
   lane pairs and on lane quads (kzg_ctx_set_reduction_lanes), at the smallest shapes that reach each kernel:
     NAF mode (per-bit tables)   n = 2^14, 2^14 + 1 (c = 13: 4 096 buckets, 64 groups) and 2^15 (c = 15: 16 384 buckets, 256 groups)
     KZG_NO_NAF (fixed windows)  the same n on the c = 15 window tables (16 384 buckets), and 2^11 coefficients (17 x 2^11 entries on
                                 16 384 buckets: the fused level)
     batched mode                5 and 512 polynomials of 512 coefficients: 64 buckets = one group per polynomial; 6 groups leave the
                                 second workgroup of four half empty
   (An SRS of 2^15 points, not 2^14: n = 2^14 + 1 needs the room, and the NAF mode reaches c = 15 from 2^15 pairs on.)
   Scalars: uniform; all equal (one heavy bucket per digit position); all zero; 2^253 - 1 beside 2^36 - 1; scalars whose every digit
   falls into bucket 63 or 64 -- the last bucket of one group and the first of the next (batched mode, 64 buckets per polynomial:
   buckets 63 and 0).
"""
import ctypes as C
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import pyref
from pyref import R_

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
DC = os.path.join(HERE, "devcheck")
TAU = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % R_
G = (1, 2)
N_SRS = 1 << 15
KINDS = ("uniform", "all equal", "all zero", "2^253 - 1 beside 2^36 - 1", "buckets 63 and 64")


def build_treecheck():
    exe = os.path.join(DC, "treecheck")
    deps = [os.path.join(DC, "treecheck.hip")] + [os.path.join(CSRC, f) for f in ("field29.h", "fe_asm.h", "field_constants.h", "curve.h", "curve_pair.h",
                                                                                    "curve_quad.h", "host_curve.h")]
    if not (os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps)):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + CSRC, deps[0], "-o", exe + ".tmp"], timeout=600)
        os.replace(exe + ".tmp", exe)
    return exe


def test_tree_on_its_own_pairs_and_quads():
    r = subprocess.run([build_treecheck()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "treecheck ok", (r.returncode, r.stdout[-500:], r.stderr[-3000:])


# ----- through the C-ABI ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


@pytest.fixture(scope="module")
def tau_powers():
    tp = [1] * N_SRS
    for i in range(1, N_SRS):
        tp[i] = tp[i - 1] * TAU % R_
    return tp


_MULT = {}


def mult(s):
    s %= R_
    if s not in _MULT:
        _MULT[s] = pyref.ec_mul(s, G) if s else None
    return _MULT[s]


def fixed_window_scalar(rnd, c):
    """every c-bit window digit is 64 or 65 (buckets 63 and 64; below 2^(c-1): no carries), the top window empty"""
    return sum(rnd.choice((64, 65)) << (c * w) for w in range(254 // c - 1))


def naf_scalar(rnd, c, buckets):
    """a width-(c + 1) NAF whose digits are +-(2 key + 1) for the keys of `buckets` (naf.h naf_bucket: the key rotated right by six
    bits), at least c + 2 positions apart, the top digit positive"""
    nbits = c - 1
    keys = [((b & ((1 << (nbits - 6)) - 1)) << 6) | (b >> (nbits - 6)) for b in buckets]
    s, pos, digits = 0, 0, []
    while pos + c + 2 < 250:
        digits.append((pos, 2 * rnd.choice(keys) + 1))
        pos += c + 2 + rnd.randrange(3)
    for i, (p, d) in enumerate(digits):
        s += (d if i == len(digits) - 1 or rnd.randrange(2) else -d) << p
    assert 0 < s < R_
    return s


def scalars(kind, n, seed, boundary):
    rnd = random.Random(seed)
    if kind == "uniform":
        return [rnd.randrange(R_) for _ in range(n)]
    if kind == "all equal":
        return [rnd.randrange(R_)] * n
    if kind == "all zero":
        return [0] * n
    if kind == "2^253 - 1 beside 2^36 - 1":
        return [(1 << 253) - 1 if i % 2 == 0 else (1 << 36) - 1 for i in range(n)]
    few = [boundary(rnd) for _ in range(16)]            # (16 distinct scalars: their buckets are heavy as well)
    return [few[rnd.randrange(16)] for _ in range(n)]


def check_msms(k, srs, tau_powers, sizes, boundary_of_n, seed):
    """kzg_msm_g1_srs over srs[0 .. n) for every n of `sizes`, every kind of scalars, pairs and quads.  The scalars of the largest n are
    generated and converted once per kind (and boundary form); a smaller n takes their prefix."""
    ctx = k.default_context(); lib = k._lib.load()
    n_max = max(sizes)
    try:
        for kind in KINDS:
            cache = {}
            for n in sizes:
                key = boundary_of_n(n)[0] if kind == "buckets 63 and 64" else None
                if key not in cache:
                    c = scalars(kind, n_max, seed, boundary_of_n(n)[1])
                    prefix = [0]
                    for a, t in zip(c, tau_powers):
                        prefix.append((prefix[-1] + a * t) % R_)
                    cache[key] = (pyref.frs_to_mont(c), prefix)
                c_mont, prefix = cache[key]
                want = mult(prefix[n])
                for lanes in (2, 4):
                    ctx.set_reduction_lanes(lanes)
                    out = np.zeros(8, np.uint64); inf = C.c_uint8(0)
                    assert lib.kzg_msm_g1_srs(ctx.handle, srs.handle, 0, k._lib.ptr(c_mont), n, k._lib.ptr(out), C.byref(inf)) == 0
                    assert pyref.point_from_wire(out) == want, (kind, n, lanes)
                    assert bool(inf.value) == (want is None), (kind, n, lanes)
    finally:
        ctx.set_reduction_lanes(0)


def test_naf_mode_unfused_level(k, tau_powers):
    srs = k.SRS.generate(TAU, N_SRS)
    try:
        assert k._lib.load().kzg_srs_has_bit_tables(srs.handle, 0) == 1

        def boundary_of_n(n):                           # engine.h srs_naf_c: 13 bucket bits below 2^15 pairs, 15 from there
            c = 13 if n < (1 << 15) else 15
            return c, lambda rnd: naf_scalar(rnd, c, (63, 64))
        check_msms(k, srs, tau_powers, ((1 << 14), (1 << 14) + 1, 1 << 15), boundary_of_n, 4100)
    finally:
        srs.close()


def test_fixed_windows_unfused_and_fused_level(k, tau_powers, monkeypatch):
    monkeypatch.setenv("KZG_NO_NAF", "1")               # read when the SRS is uploaded: window tables only (c = 15 at 2^15 points)
    srs = k.SRS.generate(TAU, N_SRS)
    try:
        assert k._lib.load().kzg_srs_has_bit_tables(srs.handle, 0) == 0
        check_msms(k, srs, tau_powers, (1 << 11, 1 << 14, (1 << 14) + 1, 1 << 15), lambda n: (15, lambda rnd: fixed_window_scalar(rnd, 15)), 4200)
    finally:
        srs.close()


@pytest.mark.parametrize("count", [5, 512])
def test_batched_mode_one_group_per_polynomial(k, tau_powers, count):
    n = 512
    kzg = k.KZG.new()
    ctx = k.default_context()
    srs = k.SRS.generate(TAU, N_SRS)
    # which polynomials meet the big integers: all of a small batch; of a large one the first and last workgroups, a stretch in the
    # middle and a stride over the rest
    checked = sorted(set(range(count)) if count <= 16 else set(range(8)) | set(range(252, 260)) | set(range(count - 8, count)) | set(range(0, count, 61)))
    try:
        for kind in KINDS:
            # 64 buckets per polynomial (c = 7, width-8 NAF, bucket = key): the last bucket of a group and the first
            # (31 distinct polynomials, polynomial j = number j mod 31: every one meets every position of a workgroup of four)
            pool = [scalars(kind, n, 4300 + 7 * j, lambda rnd: naf_scalar(rnd, 7, (63, 0))) for j in range(min(count, 31))]
            pool_polys = [k.PolynomialCoeffForm(pyref.frs_to_mont(v)) for v in pool]
            rows = [pool[j % 31] for j in range(count)]
            polys = [pool_polys[j % 31] for j in range(count)]
            want = {j: mult(sum(a * t for a, t in zip(rows[j], tau_powers)) % R_) for j in checked}
            for lanes in (2, 4):
                ctx.set_reduction_lanes(lanes)
                got = kzg.commit_coeff_form_batch(polys, srs)
                assert got.shape == (count, 8)
                for j in checked:
                    assert pyref.point_from_wire(got[j]) == want[j], (kind, count, lanes, j)
    finally:
        ctx.set_reduction_lanes(0)
        srs.close()
