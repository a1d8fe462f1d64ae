"""-m gpu: batched erasure decoding (`kzg_recover_from_cosets_batch`, `KZG.recover_from_cosets_batch`).  The yardstick is the single
call on each blob with its row of indices (`kzg_recover_from_cosets`, pinned by tests/test_gpu_recover.py against tests/recover_ref.py):
every row and every flag of a batch is compared with it bit for bit (np.array_equal on the wire words), in both output forms, over the
shapes that take different paths, B = 1, 2, 7, shared and per-blob index rows, deduplicated patterns, several groups, corrupted blobs,
shortened coefficient rows, the error table, threads and contexts at once, and the bound-checked build.  The two smallest shapes are also
compared with recover_ref and with the polynomial the values were made from.

All blobs of a call share one `count`, so all missing sets of a call have one size: the pattern test runs its layout (blobs 0, 3, 5 one
set in three orders, blobs 1, 2 another, blob 4 a third, blob 6 a fourth) once with about half of the cosets missing, once with ONE coset
missing per blob and once with every coset present (seven orders of one empty pattern)."""
import ctypes as C
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

import pyref
import recover_ref
from pyref import R_

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# (n, l, count): (8, 4) m = 2, the smallest; (2048, 16) the transforms get a workspace above 2^10 points per blob; (4096, 1) half missing:
# m = 4 096 exceeds the 256-root tile (8 tiles; 8, 8 and 4 splits at 1, 2 and 7 patterns); (4096, 16) count = m: nothing missing
SHAPES = [(8, 4, 1), (64, 4, 9), (2048, 16, 70), (4096, 1, 2048), (4096, 16, 256)]
BLOBS = (1, 2, 7)


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


def random_values(shape, seed):
    """Canonical wire words of random elements below 2^252 < r: what a call interpolates need not come from a polynomial."""
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 1 << 60, size=tuple(shape) + (4,), dtype=np.uint64)


def random_rows(B, m, count, seed):
    """B rows of `count` distinct cosets in random order."""
    rnd = random.Random(seed)
    return np.array([rnd.sample(range(m), count) for _ in range(B)], dtype=np.uint64)


def single(k, ctx, ys, ks, n, l, bound, eval_form):
    """kzg_recover_from_cosets: (output, flag)."""
    L = k._lib
    ys = np.ascontiguousarray(ys, dtype=np.uint64)
    idx = np.ascontiguousarray(ks, dtype=np.uint64)
    out = np.full((n, 4), 7, dtype=np.uint64)
    flag = C.c_int32(-1)
    rc = L.load().kzg_recover_from_cosets(ctx.handle, L.ptr(ys), L.ptr(idx), len(idx), n, l, bound, eval_form, L.ptr(out), C.byref(flag))
    assert rc == 0, rc
    return out, flag.value


def singles(k, ctx, ys, idx, n, l, bound, eval_form):
    """The loop of single calls over the blobs: (B, n, 4) rows and B flags."""
    rows = [single(k, ctx, ys[b], idx if idx.ndim == 1 else idx[b], n, l, bound, eval_form) for b in range(len(ys))]
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], dtype=np.int32)


def batch(k, ctx, ys, idx, n, l, bound, eval_form, out_len=0, flags=True):
    """The C-ABI entry: (status, rows, flags); rows and flags start from a pattern the call has to overwrite."""
    L = k._lib
    ys = np.ascontiguousarray(ys, dtype=np.uint64)
    idx = np.ascontiguousarray(idx, dtype=np.uint64)
    B, count = ys.shape[0], ys.shape[1]
    out = np.full((B, out_len or n, 4), 7, dtype=np.uint64)
    fl = np.full(B, -1, dtype=np.int32)
    rc = L.load().kzg_recover_from_cosets_batch(ctx.handle, L.ptr(ys), L.ptr(idx), 1 if idx.ndim == 1 else B, B, count, n, l, bound, eval_form, out_len,
                                                L.ptr(out), fl.ctypes.data_as(C.POINTER(C.c_int32)) if flags else None)
    return rc, out, fl


# ---- 1. every blob of a batch equals the single call on it, both forms, index rows per blob and shared ----------------------------------
@pytest.mark.parametrize("B", BLOBS)
@pytest.mark.parametrize("n,l,count", SHAPES)
def test_rows_are_the_single_calls_bit_for_bit(k, n, l, count, B):
    ctx = k.default_context()
    ys = random_values((B, count, l), n + l + B)
    rows = random_rows(B, n // l, count, "%d/%d/%d" % (n, l, B))
    for idx in (rows, rows[0]):
        for form in (1, 0):
            want, want_flags = singles(k, ctx, ys, idx, n, l, 0, form)
            rc, got, flags = batch(k, ctx, ys, idx, n, l, 0, form)
            assert rc == 0 and np.array_equal(got, want) and np.array_equal(flags, want_flags) and flags.all()


# ---- 2. ... and, independently of the single call, the reference and the polynomial the values were made from ----------------------------
@pytest.mark.parametrize("n,l,count", SHAPES[:2])
def test_small_shapes_against_the_reference_and_the_polynomial(k, n, l, count):
    ctx = k.default_context()
    m, B = n // l, 3
    rows = random_rows(B, m, count, n)
    polys, ys = [], []
    for b in range(B):
        rnd = random.Random("%d/%d" % (n, b))
        f = [rnd.randrange(R_) for _ in range(count * l)] + [0] * (n - count * l)
        ev = recover_ref.fft(f)
        polys.append((f, ev))
        ys.append([[ev[int(kk) + j * m] for j in range(l)] for kk in rows[b]])
    wire = np.stack([np.stack([pyref.frs_to_mont(item) for item in blob]) for blob in ys])
    rc, coeffs, flags = batch(k, ctx, wire, rows, n, l, 0, 0)
    assert rc == 0 and flags.all()
    rc, evals, flags = batch(k, ctx, wire, rows, n, l, 0, 1)
    assert rc == 0 and flags.all()
    for b in range(B):
        f, ev = polys[b]
        assert np.array_equal(coeffs[b], pyref.frs_to_mont(f)) and np.array_equal(evals[b], pyref.frs_to_mont(ev))
        want, consistent = recover_ref.recover(n, l, [int(kk) for kk in rows[b]], ys[b], count * l)
        assert consistent and np.array_equal(coeffs[b], pyref.frs_to_mont(want))


# ---- 3. patterns: equal sets in different orders, different sets, one missing, none missing ------------------------------------------------
def pattern_rows(m, count, seed):
    """Seven rows: 0, 3, 5 one set in three orders; 1, 2 another (two orders); 4 a third; 6 a fourth.  With count = m all are the full set."""
    rnd = random.Random(seed)
    sets = []
    while len(sets) < 4:
        s = sorted(rnd.sample(range(m), count))
        if s not in sets or count == m:
            sets.append(s)
    rows = []
    for which in (0, 1, 1, 0, 2, 0, 3):
        row = list(sets[which])
        rnd.shuffle(row)
        rows.append(row)
    assert count == m or (rows[0] != rows[3] and rows[0] != rows[5] and rows[3] != rows[5])
    return np.array(rows, dtype=np.uint64)


@pytest.mark.parametrize("n,l,count", [(64, 4, 9), (64, 4, 15), (64, 4, 16), (4096, 4, 424), (4096, 4, 1023), (4096, 4, 1024)])
def test_patterns_shared_permuted_and_distinct(k, n, l, count):
    ctx = k.default_context()
    rows = pattern_rows(n // l, count, n + count)
    ys = random_values((7, count, l), count)
    for form in (1, 0):
        want, _ = singles(k, ctx, ys, rows, n, l, 0, form)
        rc, got, flags = batch(k, ctx, ys, rows, n, l, 0, form)
        assert rc == 0 and flags.all() and np.array_equal(got, want)
    # one shared row is the same row repeated
    rc, shared, _ = batch(k, ctx, ys, rows[4], n, l, 0, 1)
    rc2, repeated, _ = batch(k, ctx, ys, np.tile(rows[4], (7, 1)), n, l, 0, 1)
    assert rc == 0 and rc2 == 0 and np.array_equal(shared, repeated)
    assert np.array_equal(shared, singles(k, ctx, ys, rows[4], n, l, 0, 1)[0])


# ---- 4. groups: 3 + 3 + 1 and seven of one give the bits of the one-group call -----------------------------------------------------------
@pytest.mark.parametrize("n,l,count", [(64, 4, 9), (4096, 1, 2048)])
def test_groups_do_not_change_a_bit(k, n, l, count):
    L = k._lib
    ctx = L.Context(0)
    B = 7
    rows = pattern_rows(n // l, count, n)
    ys = random_values((B, count, l), n + 1)
    info = k.helpers.recover_batch_info(B, count, n, l)
    assert (info["blobs_per_group"], info["groups"]) == (7, 1)
    per = info["blob_bytes"]
    for idx in (rows, rows[2]):
        for form, out_len in ((1, 0), (0, 0), (0, count * l)):
            ctx.set_recover_group_bytes(0)
            rc, want, want_flags = batch(k, ctx, ys, idx, n, l, 0, form, out_len)
            assert rc == 0
            for budget, groups in ((3 * per, (3, 3)), (1, (1, 7))):
                asked = k.helpers.recover_batch_info(B, count, n, l, out_len, budget)
                assert (asked["blobs_per_group"], asked["groups"]) == groups and asked["group_bytes"] == groups[0] * per + 16
                ctx.set_recover_group_bytes(budget)
                rc, got, flags = batch(k, ctx, ys, idx, n, l, 0, form, out_len)
                assert rc == 0 and np.array_equal(got, want) and np.array_equal(flags, want_flags)
    with pytest.raises(ValueError):
        ctx.set_recover_group_bytes(-1)
    ctx.close()


# ---- 5. one flag per blob -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,l,count", [(64, 4, 8), (4096, 16, 100)])
def test_flags_name_the_corrupted_blobs(k, n, l, count):
    L = k._lib
    ctx = k.default_context()
    m, d, B = n // l, count * l // 2, 7                               # degree < count l / 2: twice the cosets it needs
    rows = random_rows(B, m, count, n + 5)
    kz = k.KZG.new()
    ys = []
    for b in range(B):
        coeffs = np.zeros((n, 4), dtype=np.uint64)
        coeffs[:d] = random_values((d,), n + b)
        cosets = kz.cosets(k.PolynomialCoeffForm(coeffs).to_eval_form(), l)
        ys.append(cosets[rows[b].astype(np.int64)])
    ys = np.ascontiguousarray(np.stack(ys))
    rc, clean, flags = batch(k, ctx, ys, rows, n, l, d, 0)
    assert rc == 0 and flags.tolist() == [1] * B and not clean[:, d:].any()
    for b in (2, 5):                                                   # one value changed
        ys[b, count // 2, l - 1] = pyref.fr_to_mont(pyref.fr_from_mont(ys[b, count // 2, l - 1]) + 1)
    for form in (0, 1):
        want, want_flags = singles(k, ctx, ys, rows, n, l, d, form)
        rc, got, flags = batch(k, ctx, ys, rows, n, l, d, form)
        assert rc == 0 and flags.tolist() == [1, 1, 0, 1, 1, 0, 1] == want_flags.tolist()
        assert np.array_equal(got, want)                               # the corrupted rows are still the single call's interpolant
        rc, no_flags, _ = batch(k, ctx, ys, rows, n, l, d, form, flags=False)                  # out_consistent = NULL
        assert rc == 0 and np.array_equal(no_flags, want)
    # the Python surface returns the flags and does not raise
    out, consistent = kz.recover_from_cosets_batch(rows, ys, n, degree_bound=d, eval_form=False)
    assert consistent.dtype == bool and consistent.tolist() == [True, True, False, True, True, False, True]
    assert np.array_equal(out, singles(k, ctx, ys, rows, n, l, d, 0)[0])
    out, consistent = kz.recover_from_cosets_batch(rows[0], ys[:1], n)
    assert out.shape == (1, n, 4) and consistent.tolist() == [True]


# ---- 6. out_len: the first coefficients only; the flag still covers the rest ----------------------------------------------------------------
@pytest.mark.parametrize("n,l,count", [(64, 4, 8), (4096, 16, 100)])
def test_out_len_keeps_the_first_coefficients_and_the_whole_flag(k, n, l, count):
    ctx = k.default_context()
    m, B = n // l, 7
    d = count * l // 2
    rows = random_rows(B, m, count, n + 6)
    ys = random_values((B, count, l), n + 6)                           # generic values: degree count l - 1, a nonzero coefficient at every index >= d
    rc, full, full_flags = batch(k, ctx, ys, rows, n, l, d, 0)
    assert rc == 0 and not full_flags.any() and full[:, count * l - 1].any()
    for out_len in (d, d + 1, count * l, n - 1, n):
        rc, got, flags = batch(k, ctx, ys, rows, n, l, d, 0, out_len)
        assert rc == 0 and got.shape == (B, out_len, 4) and np.array_equal(got, full[:, :out_len])
        assert not flags.any()                                         # the nonzero coefficients sit at indices >= out_len = d too
    zero = np.zeros((B, count, l, 4), dtype=np.uint64)                 # ... and a consistent batch keeps its flags
    rc, got, flags = batch(k, ctx, zero, rows, n, l, d, 0, d)
    assert rc == 0 and flags.all() and not got.any()
    # polynomials of degree < d, except that blob 3 has ONE more coefficient, at count l - 1: beyond the d + 1 coefficients that leave
    kz = k.KZG.new()
    low = []
    for b in range(B):
        coeffs = np.zeros((n, 4), dtype=np.uint64)
        coeffs[:d] = random_values((d,), n + 60 + b)
        if b == 3:
            coeffs[count * l - 1] = pyref.fr_to_mont(5)
        low.append(kz.cosets(k.PolynomialCoeffForm(coeffs).to_eval_form(), l)[rows[b].astype(np.int64)])
    low = np.ascontiguousarray(np.stack(low))
    rc, got, flags = batch(k, ctx, low, rows, n, l, d, 0, d + 1)
    assert rc == 0 and flags.tolist() == [1, 1, 1, 0, 1, 1, 1] and not got[:, d].any()
    assert np.array_equal(got, batch(k, ctx, low, rows, n, l, d, 0)[1][:, :d + 1])
    for out_len in (1, d - 1, n + 1):                                  # below the bound, above n
        assert batch(k, ctx, ys, rows, n, l, d, 0, out_len)[0] == k._lib.ERR_INVALID_ARG
    for out_len in (d, n - 1, n + 1):                                  # evaluations come whole
        assert batch(k, ctx, ys, rows, n, l, d, 1, out_len)[0] == k._lib.ERR_INVALID_ARG
    rc, ev, _ = batch(k, ctx, ys, rows, n, l, d, 1, n)
    assert rc == 0 and np.array_equal(ev, batch(k, ctx, ys, rows, n, l, d, 1)[1])
    kz = k.KZG.new()
    out, consistent = kz.recover_from_cosets_batch(rows, ys, n, degree_bound=d, eval_form=False, out_len=d)
    assert np.array_equal(out, full[:, :d]) and not consistent.any()
    with pytest.raises(k.errors.GenericError):
        kz.recover_from_cosets_batch(rows, ys, n, degree_bound=d, out_len=d)


# ---- 7. errors, in the documented order ----------------------------------------------------------------------------------------------------
def test_error_table_then_a_bit_exact_call(k):
    L = k._lib
    lib = L.load()
    ctx = L.Context(0)
    n, l, B = 64, 4, 3
    m = n // l
    ks = np.array([[3, 0, 9, 14, 5], [1, 2, 3, 4, 5], [15, 0, 7, 8, 2]], dtype=np.uint64)
    ys = random_values((B, 5, l), 707)
    out = np.zeros((B, n, 4), dtype=np.uint64)
    flags = np.zeros(B, dtype=np.int32)

    def call(idx=ks, rows=None, blobs=B, count=None, n_=n, l_=l, bound=0, form=0, out_len=0, ctx_h=ctx.handle, ys_=ys, out_=out, null_idx=False):
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        return lib.kzg_recover_from_cosets_batch(ctx_h, None if ys_ is None else L.ptr(ys_), None if null_idx else L.ptr(idx),
                                                 (1 if idx.ndim == 1 else len(idx)) if rows is None else rows, blobs, idx.shape[-1] if count is None else count,
                                                 n_, l_, bound, form, out_len, None if out_ is None else L.ptr(out_), flags.ctypes.data_as(C.POINTER(C.c_int32)))

    assert call(ctx_h=None, rows=2) == L.ERR_INVALID_ARG                               # 1. null pointers and blobs = 0, in front of everything
    assert call(ys_=None, n_=0) == L.ERR_INVALID_ARG
    assert call(null_idx=True, n_=96) == L.ERR_INVALID_ARG
    assert call(out_=None, n_=1 << 25) == L.ERR_INVALID_ARG
    assert call(blobs=0, rows=1, n_=0) == L.ERR_INVALID_ARG
    assert call(rows=2, n_=0) == L.ERR_INVALID_ARG                                     # 2. index_rows neither 1 nor blobs, in front of n = 0
    assert call(rows=0) == L.ERR_INVALID_ARG
    assert call(n_=0) == L.ERR_NOT_POWER_OF_TWO                                        # 3. the single entry's rows 2 .. 5
    assert call(n_=96, l_=3) == L.ERR_NOT_POWER_OF_TWO
    assert call(n_=1 << 25, l_=3) == L.ERR_DOMAIN
    assert call(n_=1) == L.ERR_INVALID_ARG
    assert call(l_=0) == L.ERR_INVALID_ARG and call(l_=3) == L.ERR_INVALID_ARG and call(l_=64) == L.ERR_INVALID_ARG
    assert call(count=0) == L.ERR_INVALID_ARG and call(count=m + 1) == L.ERR_INVALID_ARG
    bad = ks.copy(); bad[2, 1] = m
    assert call(bad, bound=99) == L.ERR_INVALID_ARG                                    # 4. an index = m in the last row, in front of the bound
    bad[2, 1] = 2 ** 64 - 1
    assert call(bad) == L.ERR_INVALID_ARG
    bad = ks.copy(); bad[1, 4] = 1
    assert call(bad) == L.ERR_INVALID_ARG                                              #    a duplicate in the middle row
    assert call(bound=5 * l + 1, out_len=1) == L.ERR_INVALID_ARG                       # 5. too few cosets, in front of out_len
    assert call(out_len=5 * l - 1) == L.ERR_INVALID_ARG                                # 6. out_len below the bound, above n, or with evaluations
    assert call(out_len=n + 1) == L.ERR_INVALID_ARG
    assert call(form=1, out_len=n - 1) == L.ERR_INVALID_ARG
    one = np.zeros((1, 1, 1, 4), dtype=np.uint64)                                     # 7. the cap: refused before anything is allocated or read
    assert call([0], blobs=1, n_=1 << 24, l_=1, ys_=one, out_=one) == L.ERR_TOO_LARGE
    assert call([0], blobs=1, n_=1 << 24, l_=1, out_len=2, form=1, ys_=one, out_=one) == L.ERR_INVALID_ARG      # 6 in front of 7
    assert call([0], blobs=2 ** 64 - 1, n_=1 << 24, l_=1, ys_=one, out_=one) == L.ERR_TOO_LARGE                  # 7 in front of 8
    assert call(ks[0], blobs=2 ** 64 // (n * 32) + 1) == L.ERR_INVALID_ARG             # 8. the batch's arrays overflow size_t
    assert not out.any() and not flags.any()
    # the Python surface
    kz = k.KZG.new(ctx)
    bad = ks.copy(); bad[1, 4] = 1
    with pytest.raises(k.errors.GenericError):
        kz.recover_from_cosets_batch(bad, ys, n)
    with pytest.raises(k.errors.GenericError):
        kz.recover_from_cosets_batch(ks, ys, n, degree_bound=5 * l + 1)
    with pytest.raises(k.errors.GenericError):
        kz.recover_from_cosets_batch(ks[:2], ys, n)
    # the context is as usable as before
    want, _ = singles(k, ctx, ys, ks, n, l, 0, 0)
    assert call() == 0 and flags.all() and np.array_equal(out, want)
    ctx.close()


# ---- 8. two threads on one context, a second context beside them ---------------------------------------------------------------------------
def test_threads_and_contexts_at_once(k):
    cases = {}
    ctx0 = k.default_context()
    for name, (n, l, count, B) in {"a": (1024, 4, 130, 5), "b": (512, 1, 300, 3), "c": (2048, 32, 33, 4)}.items():
        rows = random_rows(B, n // l, count, name)
        ys = random_values((B, count, l), len(name) + n)
        cases[name] = (n, rows, ys, {form: singles(k, ctx0, ys, rows, n, l, 0, form)[0] for form in (0, 1)})
    ctx_a, ctx_b = k._lib.Context(0), k._lib.Context(0)
    kz_a, kz_b = k.KZG.new(ctx_a), k.KZG.new(ctx_b)
    errors, results = [], {}

    def run(name, kz, eval_form):
        try:
            n, rows, ys = cases[name][:3]
            results[name] = [kz.recover_from_cosets_batch(rows, ys, n, eval_form=eval_form) for _ in range(4)]
        except Exception as e:                                      # reported below
            errors.append((name, repr(e)))

    ts = [threading.Thread(target=run, args=a) for a in (("a", kz_a, True), ("b", kz_a, False), ("c", kz_b, True))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for name, form in (("a", 1), ("b", 0), ("c", 1)):
        assert all(np.array_equal(out, cases[name][3][form]) and flags.all() for out, flags in results[name])
    ctx_a.close(); ctx_b.close()


# ---- 9. the bound-checked build runs the small cases above with every site counter at 0 ----------------------------------------------------
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
rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", "-x", "tests/test_gpu_recover_batch.py", "-k",
                  "rows_are_the_single_calls or patterns_shared or groups_do_not or out_len_keeps"])
counts = (C.c_ulonglong * n)()
first = (C.c_int32 * (9 * n))()
assert h.kzg_bc_read_all(counts, first) == 0
print("PYTEST_RC", int(rc))
for s in range(n):
    print("SITE", s, counts[s])
'''


def test_bound_checked_build_keeps_every_precondition():
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "PYTEST_RC 0" in out, (out[-3000:], res.stderr[-2000:])
    assert " passed" in out and "no tests ran" not in out, out[-1000:]
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert sites
    fired = {int(s[1]): int(s[2]) for s in sites if int(s[2])}
    assert not fired, fired
