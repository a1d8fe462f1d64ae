"""-m gpu: the headers of many blobs in one call (`kzg_commit_with_length_proof_batch`) and the batched G2 MSM over shared bases
(`kzg_msm_g2_srs_batch`).  Setup of order N = 2^16 with a known tau, as tests/test_gpu_length_proof.py.  The contract is equality with
the loop of single calls, bit for bit, on all three outputs: lengths that are no power of two (in-blob indexing), both sides of a
window-width change and of the 2^18-entry sort switch, groups of 2, 2, 1 under a cap, degenerate blobs among random ones, identity bases, a
non-zero offset, groups of one, closed forms over two different base sets (single call and batch: the single call is the batch of one), the
three-kernel scan of the bucket counts (33 blobs of 2^14 coefficients, against the closed forms), the error table in
its documented order, accept / reject through the batched verifier, and the same kernels in the bound-checked build.  `helpers.g2_batch_info`
proves that a shape takes the path the test means.  Every test with more than one blob fails if the accumulate indexed blob * n + i into
the shared bases."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import rust_kzg_bn254_amd as k
from pyref import R_
from rust_kzg_bn254_amd import _lib, helpers, verifier
from rust_kzg_bn254_amd.errors import FFTError, SrsCapacityExceeded
from rust_kzg_bn254_amd.fr import fr_from_int, frs_from_ints

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VARIANT = os.path.join(ROOT, "rust-kzg-bn254_amd", "libkzg_bn254_mi355x_boundcheck.so")
N_SITES = 14
TAU = 0x2B992DDFA23249D6A1B5C4D3E2F10987
N = 1 << 16
TRAIL = 1 << 12
SHAPES = [(1, 1), (5, 8), (1000, 1024), (2047, 2048), (2048, 2048), (4096, 4096)]


def make_setup(points):
    g1 = k.SRS.generate(TAU, points)
    g2 = k.G2SRS.generate(TAU, points)
    trailing = k.G2SRS.generate(TAU, points, first_power=N - points)
    return g1, g2, trailing


@pytest.fixture(scope="module")
def setup():
    hs = make_setup(TRAIL)
    yield hs
    for h in hs:
        h.close()


def shift_g1(d):
    s = k.SRS.generate(TAU, 1, first_power=N - d)
    try:
        return s.g1[0].copy()
    finally:
        s.close()


_blobs = {}
_singles = {}


def blobs_of(n, count=5):
    """the same `count` random blobs of n coefficients for every test: (count, n, 4) wire words"""
    if n not in _blobs:
        rnd = random.Random(1000 + n)
        _blobs[n] = np.ascontiguousarray(frs_from_ints([rnd.randrange(R_) for _ in range(count * n)]).reshape(count, n, 4))
    return _blobs[n]


def single(setup, coeffs, d, key=None):
    """the single call on one blob (computed once per key)"""
    if key is not None and key in _singles:
        return _singles[key]
    g1, g2, trailing = setup
    out = k.KZG.new().commit_with_length_proof(k.PolynomialCoeffForm(np.ascontiguousarray(coeffs)), g1, g2, trailing, N, d)
    if key is not None:
        _singles[key] = out
    return out


def loop(setup, rows, d, key=None):
    outs = [single(setup, rows[b], d, None if key is None else (key, b)) for b in range(len(rows))]
    return tuple(np.stack([o[j] for o in outs]) for j in range(3))


def batch(setup, rows, d):
    g1, g2, trailing = setup
    return k.KZG.new().commit_with_length_proof_batch(list(rows), g1, g2, trailing, N, d)


def assert_rows_equal(got, want):
    for name, a, b in zip(("commitment", "length commitment", "length proof"), got, want):
        assert a.shape == b.shape and np.array_equal(a, b), name


@pytest.mark.parametrize("B", [1, 2, 5])
@pytest.mark.parametrize("n,d", SHAPES)
def test_rows_equal_the_loop_of_single_calls(setup, n, d, B):
    rows = blobs_of(n)[:B]
    info = helpers.g2_batch_info(n, 2, B)
    assert info["batched"] and info["blobs_per_group"] == B and info["groups"] == 1            # one group: the batched kernels carry every blob
    if n == 4096:                                                                              # either side of the 2^18-entry sort switch
        assert info["sort_small"] == (1 if B == 1 else 0) and (info["entries"] < 1 << 18) == (B == 1)
    if n in (2047, 2048):                                                                      # either side of a window-width change
        assert info["c"] == (4 if n == 2047 else 5)
    got = batch(setup, rows, d)
    assert got[0].shape == (B, 8) and got[1].shape == (B, 16) and got[2].shape == (B, 16)
    assert_rows_equal(got, loop(setup, rows, d, key=(n, d)))


def test_msm_batch_equals_the_loop_at_a_non_zero_offset(setup):
    _, _, trailing = setup
    lib, ctx = _lib.load(), _lib.default_context()
    n, B, offset = 1000, 3, 77
    rows = blobs_of(n)[:B]
    got = trailing.msm_batch(rows, offset=offset)
    want = np.zeros((B, 16), np.uint64)
    for b in range(B):
        inf = C.c_uint8(0)
        assert lib.kzg_msm_g2_srs(ctx.handle, trailing.handle, offset, _lib.ptr(np.ascontiguousarray(rows[b])), n, _lib.ptr(want[b]), C.byref(inf)) == _lib.OK
    assert np.array_equal(got, want) and want.any()
    # the flags, and the scalars already on the device
    import torch
    d_rows = torch.from_numpy(rows.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    out = np.zeros((B, 16), np.uint64); flags = np.full(B, 7, np.uint8)
    assert lib.kzg_msm_g2_srs_batch_device(ctx.handle, trailing.handle, offset, C.c_void_p(d_rows.data_ptr()), n, B, _lib.ptr(out),
                                           flags.ctypes.data_as(_lib.u8p)) == _lib.OK
    assert np.array_equal(out, want) and not flags.any()
    with pytest.raises(k.errors.GenericError):
        trailing.msm_batch(rows, offset=TRAIL - n + 1)                                         # offset + n > len: KZG_ERR_POLY_LENGTH


def test_groups_under_a_cap_give_the_same_bits(setup):
    n, d, B = 1000, 1024, 5
    rows = blobs_of(n)[:B]
    info = helpers.g2_batch_info(n, 2, B, max_blobs=2)
    assert info["groups"] == 3 and info["blobs_per_group"] == 2 and info["batched"]
    ctx = _lib.default_context()
    want = batch(setup, rows, d)
    ctx.set_g2_batch_group(2)
    try:
        got = batch(setup, rows, d)                                                            # groups of 2, 2, 1
    finally:
        ctx.set_g2_batch_group(0)
    assert_rows_equal(got, want)
    assert_rows_equal(got, loop(setup, rows, d, key=(n, d)))


def test_groups_of_one_give_the_same_bits(setup):
    n, d, B = 300, 512, 3
    rows = blobs_of(n)[:B]
    info = helpers.g2_batch_info(n, 2, B, max_blobs=1)
    assert info["groups"] == 3 and info["blobs_per_group"] == 1 and info["batched"]
    ctx = _lib.default_context()
    want = batch(setup, rows, d)                                                               # one group of three
    ctx.set_g2_batch_group(1)
    try:
        got = batch(setup, rows, d)
    finally:
        ctx.set_g2_batch_group(0)
    assert_rows_equal(got, want)


# ---- closed forms over two DIFFERENT base sets: since the single call is the batch of one, "batch = loop of single calls" compares one
# implementation with itself; here both are compared with [sum a_i s_i] G2 and [sum a_i t_i] G2 for known s_i != t_i
CF_MAX = 2048
CF_SHAPES = [(64, 64), (300, 512), (2048, 2048)]           # lane cap inactive; active with c = 4; c = 5


@pytest.fixture(scope="module")
def two_sets():
    """CF_MAX bases [s_i] G2 and CF_MAX bases [t_i] G2 with known s_i != t_i (computed once, never modified)"""
    rnd = random.Random(4242)
    s = [rnd.randrange(1, R_) for _ in range(CF_MAX)]
    t = [rnd.randrange(1, R_) for _ in range(CF_MAX)]
    assert all(x != y for x, y in zip(s, t))
    ps = np.stack([helpers.g2_mul_generator(fr_from_int(v)) for v in s])
    pt = np.stack([helpers.g2_mul_generator(fr_from_int(v)) for v in t])
    ps.setflags(write=False); pt.setflags(write=False)
    g1 = k.SRS.generate(TAU, CF_MAX)
    yield s, t, ps, pt, g1
    g1.close()


def g2_of(total):
    return helpers.g2_mul_generator(fr_from_int(total % R_)) if total % R_ else np.zeros(16, np.uint64)


@pytest.mark.parametrize("n,d", CF_SHAPES)
def test_single_and_batch_match_the_closed_forms_over_two_base_sets(two_sets, n, d):
    s, t, ps, pt, g1 = two_sets
    dead = sorted({0, 63, 64, n - 1} & set(range(n)))                                          # identity bases in set 1 only
    pts1 = np.array(pt[:d])
    pts1[dead] = 0
    t_live = [0 if i in dead else t[i] for i in range(n)]
    assert helpers.g2_batch_info(n, 2, 1)["c"] == {64: 4, 300: 4, 2048: 5}[n]
    info = helpers.g2_batch_info(n, 2, 1)
    assert (info["nl"] == -(-4 * info["G"] // 256) * 256 < -(-info["entries"] // 4)) == (n != 64)          # the lane cap binds, or does not
    rnd = random.Random(500 + n)
    ints = {"random": [rnd.randrange(R_) for _ in range(n)], "equal": [rnd.randrange(1, R_)] * n, "zero": [0] * n,
            "random2": [rnd.randrange(R_) for _ in range(n)]}
    rows = {name: frs_from_ints(a) for name, a in ints.items()}
    want = {name: (g2_of(sum(x * y for x, y in zip(a, s))), g2_of(sum(x * y for x, y in zip(a, t_live)))) for name, a in ints.items()}
    assert not want["zero"][0].any() and not want["zero"][1].any() and want["equal"][1].any()
    h0 = k.G2SRS.from_points(np.ascontiguousarray(ps[:d]))
    h1 = k.G2SRS.from_points(pts1, first_power=N - d)
    hs = (g1, h0, h1)
    try:
        for name in ints:                                                                      # the single call
            _, c2, pi2 = single(hs, rows[name], d)
            assert np.array_equal(c2, want[name][0]) and np.array_equal(pi2, want[name][1]), name
        for names in (["random"], ["zero"], ["random", "zero", "equal"], ["zero", "zero", "zero"], ["equal", "random2", "random"]):      # B = 1, 3
            _, c2, pi2 = batch(hs, [rows[x] for x in names], d)
            for b, name in enumerate(names):
                assert np.array_equal(c2[b], want[name][0]) and np.array_equal(pi2[b], want[name][1]), (names, b)
        # the identity's flag: the all-zero set over set 1, single and batched
        lib, ctx = _lib.load(), _lib.default_context()
        out = np.ones(16, np.uint64); inf = C.c_uint8(0)
        assert lib.kzg_msm_g2_srs(ctx.handle, h1.handle, 0, _lib.ptr(rows["zero"]), n, _lib.ptr(out), C.byref(inf)) == _lib.OK
        assert inf.value == 1 and not out.any()
        z3 = np.ascontiguousarray(np.stack([rows["zero"], rows["random"], rows["zero"]]))
        out3 = np.ones((3, 16), np.uint64); flags = np.full(3, 7, np.uint8)
        assert lib.kzg_msm_g2_srs_batch(ctx.handle, h1.handle, 0, _lib.ptr(z3), n, 3, _lib.ptr(out3), flags.ctypes.data_as(_lib.u8p)) == _lib.OK
        assert list(flags) == [1, 0, 1] and not out3[0].any() and not out3[2].any() and np.array_equal(out3[1], want["random"][1])
    finally:
        h0.close(); h1.close()


def test_the_query_of_one_blob_agrees_with_the_planner(tmp_path):
    """pure query, no GPU work: `kzg_msm_g2_batch_info` at count = 1 against the lines of tests/hostcheck/g2msm_plancheck.cpp"""
    exe = str(tmp_path / "g2msm_plancheck")
    csrc = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-I" + csrc, os.path.join(HERE, "hostcheck", "g2msm_plancheck.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    rows = [{f.split("=")[0]: int(f.split("=")[1]) for f in ln.split()} for ln in res.stdout.splitlines() if " count=1 max=0 " in ln]
    by_key = {(r["n"], r["nb"]): r for r in rows}
    for n in (1, 64, 257, 2047, 2048, 4096, 1 << 16, 1 << 20):
        for nb in (1, 2):
            r, got = by_key[(n, nb)], helpers.g2_batch_info(n, nb, 1)
            assert got["batched"] and got["blobs_per_group"] == 1 == r["group"] and got["groups"] == 1
            for a, b in (("c", "c"), ("W", "W"), ("G", "G"), ("entries", "entries"), ("nl", "nl"), ("seg", "seg"), ("sort_small", "small"), ("scan1", "scan1"),
                         ("launches", "launches"), ("workspace_bytes", "bytes")):
                assert got[a] == r[b], (n, nb, a)
    for nb in (1, 2):                                                                          # no two blobs of 2^22 scalars fit one launch
        got = helpers.g2_batch_info(1 << 22, nb, 3)
        assert not got["batched"] and got["blobs_per_group"] == 1 and got["groups"] == 3
        assert got["launches"] == 2 + got["sort_small"] + 1 + (1 if got["scan1"] else 3) + 1 + 6       # six behind the sort, whatever nb


def degenerate_rows():
    n = 2048
    rnd = blobs_of(n)
    equal = np.broadcast_to(fr_from_int(0x1234567890ABCDEF1234567890ABCDEF % R_), (n, 4))     # one heavy bucket per window: the whole-wave path
    pattern = frs_from_ints([(0, 1, R_ - 1)[i % 3] for i in range(n)])
    return np.ascontiguousarray(np.stack([np.zeros((n, 4), np.uint64), equal, pattern, rnd[0], rnd[0]]))


def test_degenerate_blobs_among_random_ones(setup):
    rows = degenerate_rows()
    got = batch(setup, rows, 2048)
    assert_rows_equal(got, loop(setup, rows, 2048))
    assert not got[0][0].any() and not got[1][0].any() and not got[2][0].any()                # the zero blob: three identities
    for j in range(3):
        assert got[j][1].any() and got[j][2].any()
        assert np.array_equal(got[j][3], got[j][4])                                            # identical blobs, identical rows


def test_identity_bases(setup):
    _, g2, _ = setup
    lib, ctx = _lib.load(), _lib.default_context()
    n, B = 64, 3
    pts = g2.g2[:n].copy()
    pts[0] = 0
    pts[7] = 0
    h = k.G2SRS.from_points(pts)
    try:
        rows = blobs_of(n)[:B]
        got = h.msm_batch(rows)
        for b in range(B):
            want = np.zeros(16, np.uint64); inf = C.c_uint8(0)
            assert lib.kzg_msm_g2_srs(ctx.handle, h.handle, 0, _lib.ptr(np.ascontiguousarray(rows[b])), n, _lib.ptr(want), C.byref(inf)) == _lib.OK
            assert np.array_equal(got[b], want) and want.any()
    finally:
        h.close()


def test_many_blobs_take_the_three_kernel_scan_and_match_the_closed_forms():
    n = d = 1 << 14
    B = 33
    info = helpers.g2_batch_info(n, 2, B)
    assert info["batched"] and info["groups"] == 1 and info["c"] == 8 and info["G"] == 33 * 32 * 128 and info["scan1"] == 0 and info["sort_small"] == 0
    rnd = random.Random(14)
    ints = [[rnd.randrange(R_) for _ in range(n)] for _ in range(B)]
    rows = [frs_from_ints(r) for r in ints]
    hs = make_setup(n)
    try:
        c, c2, pi2 = batch(hs, rows, d)
    finally:
        for h in hs:
            h.close()
    shift = pow(TAU, N - d, R_)
    for b in range(B):
        ft = 0
        for v in reversed(ints[b]):
            ft = (ft * TAU + v) % R_
        assert np.array_equal(c2[b], helpers.g2_mul_generator(fr_from_int(ft))), b              # [f_b(tau)]_2
        assert np.array_equal(pi2[b], helpers.g2_mul_generator(fr_from_int(ft * shift % R_))), b  # [tau^(N-d) f_b(tau)]_2
    sg = shift_g1(d)
    for b in (0, 16, 32):
        assert verifier.verify_length_proof(c[b], c2[b], pi2[b], sg)


def test_errors_in_the_documented_order(setup):
    g1, g2, trailing = setup
    ctx = _lib.default_context()
    lib = _lib.load()
    B = 2
    sc = np.ascontiguousarray(frs_from_ints(list(range(1, 8 * B + 1))))
    c = np.full((B, 8), 5, np.uint64); c2 = np.full((B, 16), 5, np.uint64); pi2 = np.full((B, 16), 5, np.uint64)

    def call(g1h=g1.handle, g2h=g2.handle, trh=trailing.handle, first=N - TRAIL, order=N, n=8, count=B, d=8, scalars=sc, out=c):
        return lib.kzg_commit_with_length_proof_batch(ctx.handle, g1h, g2h, trh, first, order, None if scalars is None else _lib.ptr(scalars), n, count, d,
                                                      None if out is None else _lib.ptr(out), _lib.ptr(c2), _lib.ptr(pi2))
    assert call() == _lib.OK
    # 1. null pointers win over everything else (here: over a count that is too large and an order that is no power of two)
    assert call(g1h=None, count=(1 << 20) + 1, order=3) == _lib.ERR_INVALID_ARG
    assert call(trh=None, d=3) == _lib.ERR_INVALID_ARG
    assert call(scalars=None, order=3) == _lib.ERR_INVALID_ARG
    assert call(out=None, d=5) == _lib.ERR_INVALID_ARG
    # 2. the size of the batch, before the powers of two
    assert call(count=(1 << 20) + 1, order=3) == _lib.ERR_TOO_LARGE
    assert call(n=1 << 60, count=1 << 20, order=3) == _lib.ERR_INVALID_ARG
    # 3. rows 2 to 5 of the single call: powers of two, before the size relations
    assert call(order=N - 1, n=9, d=8) == _lib.ERR_NOT_POWER_OF_TWO
    assert call(d=12, n=13) == _lib.ERR_NOT_POWER_OF_TWO
    assert call(d=0, n=0) == _lib.ERR_NOT_POWER_OF_TWO
    #    n > claimed_len, claimed_len > srs_order -- before the window check
    assert call(n=8, d=4, first=N) == _lib.ERR_INVALID_ARG
    assert call(order=4, d=8, first=N) == _lib.ERR_INVALID_ARG
    #    the window [N - d, N) inside the trailing handle -- before the length check
    tiny1 = k.SRS.generate(TAU, 4); tiny2 = k.G2SRS.generate(TAU, 4)
    try:
        assert call(d=2 * TRAIL, g1h=tiny1.handle) == _lib.ERR_SRS_CAPACITY_EXCEEDED
        assert call(first=N - 2 * TRAIL, g1h=tiny1.handle) == _lib.ERR_SRS_CAPACITY_EXCEEDED
        assert call(order=2 * N, g2h=tiny2.handle) == _lib.ERR_SRS_CAPACITY_EXCEEDED
        #    n larger than either monomial SRS
        assert call(g1h=tiny1.handle) == _lib.ERR_POLY_LENGTH
        assert call(g2h=tiny2.handle) == _lib.ERR_POLY_LENGTH
        assert call(g1h=tiny1.handle, g2h=tiny2.handle, n=4) == _lib.OK
    finally:
        tiny1.close(); tiny2.close()
    # the batched MSM: its own table
    out = np.zeros((B, 16), np.uint64)
    msm = lambda srs=g2.handle, offset=0, n=8, count=B, scalars=sc, o=out: lib.kzg_msm_g2_srs_batch(
        ctx.handle, srs, offset, None if scalars is None else _lib.ptr(scalars), n, count, None if o is None else _lib.ptr(o), None)
    assert msm() == _lib.OK
    assert msm(srs=None, count=(1 << 20) + 1) == _lib.ERR_INVALID_ARG and msm(o=None, offset=TRAIL) == _lib.ERR_INVALID_ARG
    assert msm(count=(1 << 20) + 1, offset=TRAIL) == _lib.ERR_TOO_LARGE and msm(n=1 << 60, count=1 << 20) == _lib.ERR_INVALID_ARG
    assert msm(offset=TRAIL - 7) == _lib.ERR_POLY_LENGTH and msm(offset=TRAIL + 1, n=0) == _lib.ERR_POLY_LENGTH
    # a slot-0 begin in flight refuses every G2 call
    g1s = np.ascontiguousarray(sc[:8])
    assert lib.kzg_msm_g1_srs_begin(ctx.handle, g1.handle, 0, _lib.ptr(g1s), 8, 0) == _lib.OK
    try:
        assert call() == _lib.ERR_INVALID_ARG and msm() == _lib.ERR_INVALID_ARG
    finally:
        pt = np.zeros(8, np.uint64); inf = C.c_uint8(0)
        assert lib.kzg_msm_g1_srs_end(ctx.handle, 0, _lib.ptr(pt), C.byref(inf), None) == _lib.OK
    # the Python surface maps them as its neighbours do
    kzg = k.KZG.new()
    polys = [k.PolynomialCoeffForm(np.ascontiguousarray(sc[:8])), k.PolynomialCoeffForm(np.ascontiguousarray(sc[8:]))]
    with pytest.raises(FFTError):
        kzg.commit_with_length_proof_batch(polys, g1, g2, trailing, N, 12)
    with pytest.raises(SrsCapacityExceeded):
        kzg.commit_with_length_proof_batch(polys, g1, g2, trailing, N, 2 * TRAIL)
    # count = 0 writes nothing; n = 0 writes identities (zeros, flags 1)
    c[:] = 5; c2[:] = 5; pi2[:] = 5; out[:] = 5
    assert call(count=0) == _lib.OK and (c == 5).all() and (c2 == 5).all() and (pi2 == 5).all()
    assert msm(count=0) == _lib.OK and (out == 5).all()
    assert call(n=0, scalars=None) == _lib.OK and not c.any() and not c2.any() and not pi2.any()
    flags = np.zeros(B, np.uint8)
    assert lib.kzg_msm_g2_srs_batch(ctx.handle, g2.handle, 0, None, 0, B, _lib.ptr(out), flags.ctypes.data_as(_lib.u8p)) == _lib.OK
    assert not out.any() and (flags == 1).all()
    # the context is usable after all of that
    assert call() == _lib.OK and c.any() and c2.any() and pi2.any()
    assert_rows_equal((c, c2, pi2), loop(setup, sc.reshape(B, 8, 4), 8))


def test_the_batched_verifier_accepts_the_headers_and_rejects_swapped_proofs(setup):
    n, d, B = 1000, 1024, 5
    c, c2, pi2 = batch(setup, blobs_of(n)[:B], d)
    shifts = {d: shift_g1(d)}
    assert verifier.verify_length_proof_batch(c, c2, pi2, [d] * B, shifts)
    swapped = pi2.copy()
    swapped[[1, 3]] = swapped[[3, 1]]
    assert not verifier.verify_length_proof_batch(c, c2, swapped, [d] * B, shifts)


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
WORKLOAD = ["tests/test_gpu_header_commit_batch.py::test_rows_equal_the_loop_of_single_calls[2048-2048-5]",
            "tests/test_gpu_header_commit_batch.py::test_degenerate_blobs_among_random_ones"]


def test_batched_kernels_stay_inside_every_precondition():
    """the (2048, 2048) x 5 equality case and the degenerate blobs in a child process on the bound-checked build: every counter 0"""
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    body = CHILD % {"root": ROOT, "sites": N_SITES, "tests": WORKLOAD}
    res = subprocess.run([sys.executable, "-c", body], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "PYTEST_RC 0" in out and "2 passed" in out, (out[-3000:], res.stderr[-2000:])
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert len(sites) == N_SITES
    fired = [(int(s[1]), int(s[2]), s[3:]) for s in sites if int(s[2]) != 0]
    assert not fired, "bound violations on the device (site, count, first operand limbs): %r" % (fired,)
