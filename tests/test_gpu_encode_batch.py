"""-m gpu: the batched encoder (`kzg_encode_cosets_batch`, `KZG.encode_cosets_batch`): B blobs of one shape in one call, row b of every
output bit-identical to `kzg_encode_cosets` on blob b -- the loop of single calls is the reference of every test here (that entry is
pinned against `kzg_compute_multiproofs`, known-tau closed forms and the oracle in test_gpu_encode.py).  Shapes that take every batched
kernel (direct stages and radix-2, on lanes and on pairs, the padding copy, the spread load, W > 1 in the linear combination), groups
driven by `Context.set_encode_group_bytes`, degenerate blobs among random ones, the error table, threads and contexts at once, and the
bound-checked build.  Bit-exact: np.array_equal on the wire limbs."""
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

import pyref
from pyref import R_

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G1 = (1, 2)
TAU = int.from_bytes(__import__("hashlib").sha256(b"kzg-bn254-mi355x/encode-batch/v1").digest(), "big") % R_
SENTINEL = 7


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


@pytest.fixture(scope="module")
def ref_srs(k, test_srs_wire):
    return k.SRS(test_srs_wire, order=3000)


def rand_ints(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R_) for _ in range(n)]


def blobs_of(ints_rows):
    return np.ascontiguousarray(np.stack([np.asarray(pyref.frs_to_mont(r), dtype=np.uint64).reshape(-1, 4) for r in ints_rows]))


def rand_blobs(B, d, seed):
    """(B, d, 4) wire elements of B distinct random polynomials, and their integers"""
    rows = [rand_ints(d, 100003 * seed + b) for b in range(B)]
    return blobs_of(rows), rows


def raw_single(k, srs, data, eval_form, n, l, values=True, proofs=True):
    L = k._lib
    data = np.ascontiguousarray(data, dtype=np.uint64).reshape(-1, 4)
    d, m = data.shape[0], n // l
    ys = np.full((m, l, 4), SENTINEL, dtype=np.uint64)
    out = np.full((m, 8), SENTINEL, dtype=np.uint64)
    inf = np.full(m, SENTINEL, dtype=np.uint8)
    rc = L.load().kzg_encode_cosets(srs.ctx.handle, srs.handle, L.ptr(data), d, eval_form, n, l, L.ptr(ys) if values else None,
                                    L.ptr(out) if proofs else None, inf.ctypes.data_as(L.u8p))
    assert rc == 0, (rc, srs.ctx.last_error())
    return ys, out, inf


def the_loop(k, srs, blobs, eval_form, n, l, values=True, proofs=True):
    """the reference: kzg_encode_cosets on every blob, stacked"""
    rows = [raw_single(k, srs, b, eval_form, n, l, values, proofs) for b in blobs]
    return tuple(np.stack([r[i] for r in rows]) for i in range(3))


def raw_batch(k, srs, blobs, eval_form, n, l, values=True, proofs=True):
    L = k._lib
    blobs = np.ascontiguousarray(blobs, dtype=np.uint64)
    B, d, m = blobs.shape[0], blobs.shape[1], n // l
    ys = np.full((B, m, l, 4), SENTINEL, dtype=np.uint64)
    out = np.full((B, m, 8), SENTINEL, dtype=np.uint64)
    inf = np.full((B, m), SENTINEL, dtype=np.uint8)
    rc = L.load().kzg_encode_cosets_batch(srs.ctx.handle, srs.handle, L.ptr(blobs), B, d, eval_form, n, l, L.ptr(ys) if values else None,
                                          L.ptr(out) if proofs else None, inf.ctypes.data_as(L.u8p))
    assert rc == 0, (rc, srs.ctx.last_error())
    return ys, out, inf


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. equals the loop -------------------------------------------------------------------------------------------------------------
# (1024, 2048, 512): W > 1 in the linear combination and the sum of its partials; (512, 512, 128): r = 1
SHAPES = [(2, 4, 1, 3), (64, 128, 1, 5), (256, 2048, 16, 8), (256, 2048, 1, 4), (1024, 2048, 512, 3), (512, 512, 128, 3)]


@pytest.mark.parametrize("d,n,l,B", SHAPES)
def test_equals_the_loop(k, ref_srs, d, n, l, B):
    blobs, rows = rand_blobs(B, d, d + n + l)
    assert k.helpers.encode_batch_info(d, n, l, B)["blobs_per_group"] == B            # one group: every launch carries the B blobs
    want = the_loop(k, ref_srs, blobs, 0, n, l)
    assert same(raw_batch(k, ref_srs, blobs, 0, n, l), want)
    # eval form: the d evaluations of every blob on the d-point domain
    evals = blobs_of([pyref.dft(r) for r in rows])
    want_e = the_loop(k, ref_srs, evals, 1, n, l)
    assert same(want_e, want)
    assert same(raw_batch(k, ref_srs, evals, 1, n, l), want)
    # the Python surface: a list of polynomials, and the array with eval_form=
    kzg = k.KZG.new()
    ys, proofs = kzg.encode_cosets_batch([k.PolynomialCoeffForm(b) for b in blobs], ref_srs, n, l)
    assert ys.shape == (B, n // l, l, 4) and proofs.shape == (B, n // l, 8)
    assert np.array_equal(ys, want[0]) and np.array_equal(proofs, want[1])
    ys, proofs = kzg.encode_cosets_batch(evals, ref_srs, n, l, eval_form=True)
    assert np.array_equal(ys, want[0]) and np.array_equal(proofs, want[1])


@pytest.mark.parametrize("eval_form", [0, 1])
@pytest.mark.parametrize("l", [1, 16])
def test_zero_and_constant_blobs_among_random_ones(k, ref_srs, l, eval_form):
    d, n, B = 256, 1024, 5
    _, rows = rand_blobs(B, d, 17 + l)
    rows[1] = [0] * d                                                   # the zero polynomial
    rows[3] = [4242] * d if eval_form else [4242] + [0] * (d - 1)       # a constant
    blobs = blobs_of(rows)
    ys, out, inf = raw_batch(k, ref_srs, blobs, eval_form, n, l)
    for b, c in ((1, 0), (3, 4242)):                                    # flagged identities, the constant as every value
        assert not out[b].any() and np.all(inf[b] == 1)
        assert np.array_equal(ys[b], np.broadcast_to(np.asarray(pyref.fr_to_mont(c), dtype=np.uint64), (n // l, l, 4)))
    assert same((ys, out, inf), the_loop(k, ref_srs, blobs, eval_form, n, l))     # the neighbours untouched
    assert not np.any(inf[[0, 2, 4]])


# ---- 2. B = 1 equals the single call; each output alone ------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,l", [(256, 2048, 16), (64, 128, 1)])
def test_one_blob_equals_the_single_call(k, ref_srs, d, n, l):
    blobs, _ = rand_blobs(1, d, 21)
    ys, out, inf = raw_single(k, ref_srs, blobs[0], 0, n, l)
    assert same(raw_batch(k, ref_srs, blobs, 0, n, l), (ys[None], out[None], inf[None]))


@pytest.mark.parametrize("B", [1, 4])
def test_each_output_alone_is_identical(k, ref_srs, B):
    d, n, l = 256, 2048, 16
    blobs, _ = rand_blobs(B, d, 23)
    ys, out, inf = the_loop(k, ref_srs, blobs, 0, n, l)
    ys_v, out_v, inf_v = raw_batch(k, ref_srs, blobs, 0, n, l, proofs=False)
    assert np.array_equal(ys_v, ys) and np.all(out_v == SENTINEL) and np.all(inf_v == SENTINEL)      # nothing written for the output left out
    ys_p, out_p, inf_p = raw_batch(k, ref_srs, blobs, 0, n, l, values=False)
    assert np.array_equal(out_p, out) and np.array_equal(inf_p, inf) and np.all(ys_p == SENTINEL)
    kzg = k.KZG.new()
    assert kzg.encode_cosets_batch(blobs, ref_srs, n, l, values=False, eval_form=False)[0] is None
    assert kzg.encode_cosets_batch(blobs, ref_srs, n, l, proofs=False, eval_form=False)[1] is None


# ---- 3. groups ----------------------------------------------------------------------------------------------------------------------
def test_groups_give_the_same_rows(k, ref_srs):
    d, n, l, B = 256, 2048, 16, 7
    info = k.helpers.encode_batch_info
    one_blob = info(d, n, l, 1)["group_bytes"]
    assert info(d, n, l, B)["blobs_per_group"] == B and info(d, n, l, B)["groups"] == 1
    three = info(d, n, l, B, group_bytes=3 * one_blob + one_blob // 2)
    assert (three["blobs_per_group"], three["groups"]) == (3, 3)          # 3 + 3 + 1
    ones = info(d, n, l, B, group_bytes=1)
    assert (ones["blobs_per_group"], ones["groups"]) == (1, 7)            # never smaller than one blob
    blobs, rows = rand_blobs(B, d, 31)
    evals = blobs_of([pyref.dft(r) for r in rows])
    ctx = ref_srs.ctx
    try:
        whole = raw_batch(k, ref_srs, blobs, 0, n, l)
        assert same(whole, the_loop(k, ref_srs, blobs, 0, n, l))
        for budget in (3 * one_blob + one_blob // 2, 1):
            ctx.set_encode_group_bytes(budget)
            assert same(raw_batch(k, ref_srs, blobs, 0, n, l), whole)
            assert same(raw_batch(k, ref_srs, evals, 1, n, l), whole)
            assert np.array_equal(raw_batch(k, ref_srs, blobs, 0, n, l, proofs=False)[0], whole[0])
    finally:
        ctx.set_encode_group_bytes(0)
    assert same(raw_batch(k, ref_srs, blobs, 0, n, l), whole)


# ---- 4. every batched kernel variant runs: small d, l = 1, known tau ------------------------------------------------------------------
# (d, n, B): what the batch plan makes of them is asserted from the query below, so a later threshold change cannot silently empty a case
VARIANTS = [(1024, 2048, 2),     # direct stages on pairs, the padding copy
            (1024, 2048, 8),     # direct stages on lanes, the padding copy
            (1024, 2048, 16),    # radix-2 on pairs, the spread load
            (1024, 8192, 16)]    # radix-2 on lanes (forward, 16 x 8 192 points), the spread load
_variant_srs = {}


def check_sampled_against_the_closed_form(coeffs, n, ys, proofs, samples, seed):
    log_n = n.bit_length() - 1
    w = pyref.root_of_unity(log_n)
    f_tau = pyref.poly_eval(coeffs, TAU)
    for kk in random.Random(seed).sample(range(n), samples):
        c = pow(w, kk, R_)
        f_c = pyref.poly_eval(coeffs, c)
        s = (f_tau - f_c) * pow((TAU - c) % R_, -1, R_) % R_            # [(f(tau) - f(c)) / (tau - c)] G1
        got = None if not np.asarray(proofs[kk]).any() else pyref.point_from_wire(proofs[kk])
        assert got == (None if s == 0 else pyref.ec_mul(s, G1)), kk
        assert np.array_equal(ys[kk, 0], pyref.fr_to_mont(f_c)), kk


def test_the_variants_cover_every_form(k):
    info = k.helpers.encode_batch_info
    seen, loads = set(), set()
    for d, n, B in VARIANTS:
        i = info(d, n, 1, B)
        assert i["batched"] and i["blobs_per_group"] == B
        for t in (i["inverse"], i["forward"]):
            seen.add((t["form"], "pairs" if t["pairs"] else "lanes"))
            loads.add((t["form"], t["load"]))
    assert {("direct", "lanes"), ("direct", "pairs"), ("radix2", "pairs"), ("radix2", "lanes")} <= seen, seen
    assert ("radix2", "spread") in loads and ("direct", "pad") in loads, loads


@pytest.mark.parametrize("d,n,B", VARIANTS)
def test_every_batched_variant_equals_the_loop(k, d, n, B):
    if d not in _variant_srs:
        _variant_srs[d] = k.SRS.generate(TAU, d)
    srs = _variant_srs[d]
    blobs, rows = rand_blobs(B, d, n + B)
    got = raw_batch(k, srs, blobs, 0, n, 1)
    assert same(got, the_loop(k, srs, blobs, 0, n, 1))
    if (d, n, B) == VARIANTS[2]:                                        # 32 sampled proofs and values of one blob against the closed form
        check_sampled_against_the_closed_form(rows[B - 1], n, got[0][B - 1], got[1][B - 1], 32, 41)


# ---- 5. the error table, in the header's order, then the two new rows ----------------------------------------------------------------
def test_error_table_then_a_bit_exact_call(k, ref_srs, test_srs_wire):
    L = k._lib
    lib = L.load()
    ctx = ref_srs.ctx
    good, _ = rand_blobs(3, 64, 51)
    before = raw_batch(k, ref_srs, good, 0, 128, 2)
    big = np.zeros((1 << 12, 4), dtype=np.uint64)
    ys = np.full((1 << 12, 4), SENTINEL, dtype=np.uint64)
    out = np.full((1 << 12, 8), SENTINEL, dtype=np.uint64)
    inf = np.full(1 << 12, SENTINEL, dtype=np.uint8)
    lag = ref_srs.lagrange(64)
    other_ctx = L.Context(0)
    other_srs = k.SRS(test_srs_wire[:64], order=64, ctx=other_ctx)
    NOARG = object()

    def call(srs_h, d, n, l, count=1, data=big, ctx_h=ctx.handle, ys_p=NOARG, out_p=NOARG, inf_p=NOARG):
        rc = lib.kzg_encode_cosets_batch(ctx_h, srs_h, None if data is None else L.ptr(data), count, d, 0, n, l, L.ptr(ys) if ys_p is NOARG else ys_p,
                                         L.ptr(out) if out_p is NOARG else out_p, inf.ctypes.data_as(L.u8p) if inf_p is NOARG else inf_p)
        if rc != 0:                                                     # after each error the next valid call is bit-exact
            assert np.all(ys == SENTINEL) and np.all(out == SENTINEL) and np.all(inf == SENTINEL)
            assert same(raw_batch(k, ref_srs, good, 0, 128, 2), before)
        return rc

    h = ref_srs.handle
    # 1. null pointers, no output, proofs without flags, no blob -- in front of a length that is no power of two
    assert call(h, 3, 0, 1, ctx_h=None) == L.ERR_INVALID_ARG
    assert call(None, 3, 0, 1) == L.ERR_INVALID_ARG
    assert call(h, 3, 0, 1, data=None) == L.ERR_INVALID_ARG
    assert call(h, 3, 0, 1, ys_p=None, out_p=None) == L.ERR_INVALID_ARG
    assert call(h, 3, 0, 1, inf_p=None) == L.ERR_INVALID_ARG
    assert call(h, 3, 0, 1, count=0) == L.ERR_INVALID_ARG
    assert call(h, 64, 128, 1, count=0) == L.ERR_INVALID_ARG
    # 2. an SRS of another context, a Lagrange-basis handle -- in front of the same
    assert call(other_srs.handle, 3, 0, 1) == L.ERR_INVALID_ARG
    assert call(lag.handle, 3, 0, 1) == L.ERR_INVALID_ARG
    # 3. lengths -- in front of the domain limit
    assert call(h, 0, 64, 1) == L.ERR_NOT_POWER_OF_TWO
    assert call(h, 48, 1 << 25, 1) == L.ERR_NOT_POWER_OF_TWO
    assert call(h, 64, 0, 1) == L.ERR_NOT_POWER_OF_TWO
    assert call(h, 64, 96, 1) == L.ERR_NOT_POWER_OF_TWO
    # 4. the domain limit -- in front of the shape rules
    assert call(h, 1, 1 << 25, 3) == L.ERR_DOMAIN
    # 5. shapes -- in front of the SRS capacity
    assert call(h, 4096, 2048, 1) == L.ERR_INVALID_ARG                  # poly_len > n
    assert call(h, 1, 64, 1) == L.ERR_INVALID_ARG                       # poly_len = 1
    assert call(h, 4096, 4096, 0) == L.ERR_INVALID_ARG
    assert call(h, 4096, 4096, 3) == L.ERR_INVALID_ARG                  # l not a power of two
    assert call(h, 64, 4096, 64) == L.ERR_INVALID_ARG                   # l > poly_len / 2 though l <= n / 2
    # 6. the SRS holds 3 000 points -- in front of the overflow
    assert call(h, 4096, 4096, 1) == L.ERR_SRS_CAPACITY_EXCEEDED
    assert call(h, 4096, 4096, 1, count=1 << 60) == L.ERR_SRS_CAPACITY_EXCEEDED
    assert call(other_srs.handle, 128, 256, 1, ctx_h=other_ctx.handle) == L.ERR_SRS_CAPACITY_EXCEEDED
    # 7. a count whose outputs overflow size_t
    assert call(h, 64, 128, 1, count=1 << 60) == L.ERR_INVALID_ARG
    assert call(h, 64, 128, 1, count=(1 << 64) - 1) == L.ERR_INVALID_ARG
    # flags are not needed for values alone
    assert call(h, 64, 128, 1, count=2, out_p=None, inf_p=None) == 0
    assert np.all(out == SENTINEL) and np.all(inf == SENTINEL) and not np.all(ys[:256] == SENTINEL) and np.all(ys[256:] == SENTINEL)
    assert same(raw_batch(k, ref_srs, good, 0, 128, 2), before)
    # the query: no context, the same rows 3, 4, 5, 7
    info = L.EncodeBatchInfo()
    q = lib.kzg_encode_cosets_batch_info
    import ctypes as C
    assert q(64, 128, 1, 1, 1, 1, 0, None) == L.ERR_INVALID_ARG
    assert q(64, 128, 1, 1, 0, 0, 0, C.byref(info)) == L.ERR_INVALID_ARG
    assert q(64, 128, 1, 0, 1, 1, 0, C.byref(info)) == L.ERR_INVALID_ARG
    assert q(48, 128, 1, 1, 1, 1, 0, C.byref(info)) == L.ERR_NOT_POWER_OF_TWO
    assert q(64, 1 << 25, 1, 1, 1, 1, 0, C.byref(info)) == L.ERR_DOMAIN
    assert q(64, 128, 64, 1, 1, 1, 0, C.byref(info)) == L.ERR_INVALID_ARG
    assert q(64, 128, 1, 1 << 60, 1, 1, 0, C.byref(info)) == L.ERR_INVALID_ARG
    assert q(1 << 20, 1 << 20, 1, 1, 1, 1, 0, C.byref(info)) == 0      # no SRS: no capacity row
    # the Python surface
    kzg = k.KZG.new()
    polys = [k.PolynomialCoeffForm(b) for b in good]
    with pytest.raises(k.errors.GenericError):
        kzg.encode_cosets_batch(polys, ref_srs, 256, 3)
    with pytest.raises(k.errors.GenericError):
        kzg.encode_cosets_batch([], ref_srs, 256, 1)
    with pytest.raises(k.errors.GenericError):
        kzg.encode_cosets_batch(polys + [k.PolynomialCoeffForm(big[:128])], ref_srs, 256, 1)
    with pytest.raises(TypeError):
        kzg.encode_cosets_batch(polys + [k.PolynomialEvalForm(good[0])], ref_srs, 256, 1)
    with pytest.raises(TypeError):
        kzg.encode_cosets_batch(good, ref_srs, 256, 1)                  # an array without eval_form=
    with pytest.raises(k.errors.FFTError):
        kzg.encode_cosets_batch(polys, ref_srs, 96, 1)
    with pytest.raises(k.errors.SrsCapacityExceeded):
        kzg.encode_cosets_batch([k.PolynomialCoeffForm(big)], ref_srs, 4096, 1)
    with pytest.raises(ValueError):                                     # KZG_ERR_INVALID_ARG, as everywhere in the library
        kzg.encode_cosets_batch(polys, lag, 256, 1)
    with pytest.raises(ValueError):
        ctx.set_encode_group_bytes(-1)
    assert same(raw_batch(k, ref_srs, good, 0, 128, 2), before)
    lag.close()
    other_srs.close()
    other_ctx.close()


# ---- 6. two threads on one context (the batch and the single call), a second context beside them ------------------------------------
def test_threads_and_contexts_at_once(k, test_srs_wire):
    d, n, l, B = 512, 2048, 4, 4
    blobs, _ = rand_blobs(B, d, 61)
    polys = [k.PolynomialCoeffForm(b) for b in blobs]
    ctx_a = k._lib.Context(0)
    ctx_b = k._lib.Context(0)
    srs_a = k.SRS(test_srs_wire[:d], order=d, ctx=ctx_a)
    srs_b = k.SRS(test_srs_wire[:d], order=d, ctx=ctx_b)
    kz_a, kz_b = k.KZG.new(ctx_a), k.KZG.new(ctx_b)
    # expected values, one call at a time, before anything runs concurrently
    one = k.SRS(test_srs_wire[:d], order=d)
    kz = k.KZG.new()
    want = [kz.encode_cosets(p, one, n, l) for p in polys]
    want_ys, want_proofs = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    want8 = [kz.encode_cosets(p, one, 4 * n, l) for p in polys]
    want_ys8, want_proofs8 = np.stack([w[0] for w in want8]), np.stack([w[1] for w in want8])
    one.close()
    errors, results = [], {}

    def run(name, fn):
        try:
            results[name] = fn()
        except Exception as e:                                          # reported below
            errors.append((name, repr(e)))

    def batch():                                                        # whichever of the two comes first builds the (d, l) entry on srs_a
        return [kz_a.encode_cosets_batch(polys, srs_a, n, l) for _ in range(3)]

    def single():
        return [kz_a.encode_cosets(polys[2], srs_a, n, l) for _ in range(3)]

    def other():
        return [kz_b.encode_cosets_batch(polys, srs_b, 4 * n, l) for _ in range(3)]

    ts = [threading.Thread(target=run, args=(nm, fn)) for nm, fn in (("batch", batch), ("single", single), ("other", other))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert all(np.array_equal(y, want_ys) and np.array_equal(p, want_proofs) for y, p in results["batch"])
    assert all(np.array_equal(y, want_ys[2]) and np.array_equal(p, want_proofs[2]) for y, p in results["single"])
    assert all(np.array_equal(y, want_ys8) and np.array_equal(p, want_proofs8) for y, p in results["other"])
    srs_a.close(); srs_b.close()
    ctx_a.close(); ctx_b.close()


# ---- 7. the bound-checked build runs tests 1-4 with every site counter at 0 ----------------------------------------------------------
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
WORKLOAD = ["tests/test_gpu_encode_batch.py::" + t for t in (
    "test_equals_the_loop", "test_zero_and_constant_blobs_among_random_ones", "test_one_blob_equals_the_single_call",
    "test_each_output_alone_is_identical", "test_groups_give_the_same_rows", "test_the_variants_cover_every_form",
    "test_every_batched_variant_equals_the_loop")]


def test_bound_checked_build_keeps_every_precondition():
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": WORKLOAD}], capture_output=True, text=True, timeout=1500,
                         env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "PYTEST_RC 0" in out, (out[-3000:], res.stderr[-2000:])
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert sites
    fired = {int(s[1]): int(s[2]) for s in sites if int(s[2])}
    assert not fired, fired
