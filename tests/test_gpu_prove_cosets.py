"""-m gpu: the selected-coset prover (`kzg_prove_cosets`, `kzg_coset_quotients`, `KZG.prove_cosets[_batch]`, `KZG.coset_quotients`): the
values and the proof of chosen cosets of a polynomial by one division and one commitment per coset.  Every row is compared bit for bit
(np.array_equal on the wire limbs) with the row of the encoder (`kzg_encode_cosets`) on the same polynomial; the quotients with the
big-integer synthetic division; plus degenerate polynomials, several polynomials and several groups, the protocol round trip (encode,
lose, recover, re-prove, verify), the error table in its order, and the bound-checked build."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pyref
from pyref import R_

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TAU = int.from_bytes(__import__("hashlib").sha256(b"kzg-bn254-mi355x/prove-cosets/v1").digest(), "big") % R_


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


@pytest.fixture(scope="module")
def ref_srs(k, test_srs_wire):
    return k.SRS(test_srs_wire, order=3000)


@pytest.fixture(scope="module")
def big_srs(k):
    srs = k.SRS.generate(TAU, 1 << 14)
    yield srs
    srs.close()


def rand_ints(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R_) for _ in range(n)]


def coeff_form(k, ints):
    return k.PolynomialCoeffForm(pyref.frs_to_mont(ints))


def div_xl(f, l, c):
    """f = q (X^l - c) + r: (q, r), coefficient lists (tests/test_gpu_encode.py)"""
    f = list(f)
    q = [0] * (len(f) - l)
    for i in range(len(f) - 1, l - 1, -1):
        co = f[i]
        q[i - l] = co
        f[i] = 0
        f[i - l] = (f[i - l] + co * c) % R_
    return q, f[:l]


def raw_prove(k, srs, data, count, d, eval_form, n, l, ps, ks, values=True, proofs=True):
    """the C entry on arrays filled with 7s: (rc, ys, out, inf, bad)"""
    L = k._lib
    data = np.ascontiguousarray(data, dtype=np.uint64).reshape(-1, 4)
    ks = np.ascontiguousarray(ks, dtype=np.uint64)
    ps = None if ps is None else np.ascontiguousarray(ps, dtype=np.uint64)
    ni = len(ks)
    ys = np.full((max(ni, 1), l, 4), 7, dtype=np.uint64)
    out = np.full((max(ni, 1), 8), 7, dtype=np.uint64)
    inf = np.full(max(ni, 1), 7, dtype=np.uint8)
    bad = C.c_uint64(99)
    rc = L.load().kzg_prove_cosets(srs.ctx.handle, srs.handle, L.ptr(data), count, d, eval_form, n, l, None if ps is None else L.ptr(ps), L.ptr(ks), ni,
                                   L.ptr(ys) if values else None, L.ptr(out) if proofs else None, inf.ctypes.data_as(L.u8p), C.byref(bad))
    return rc, ys, out, inf, bad.value


# ---- 1. rows equal the encoder's, on the reference's 3 000-point SRS --------------------------------------------------------------------
SHAPES = [(2, 4, 1), (64, 128, 1), (64, 128, 4), (64, 512, 32), (2048, 4096, 1), (2048, 2048, 16)]
_encoded = {}


def encoded(k, srs, d, n, l, seed=None):
    """(coeffs, ys, proofs) of the encoder on a random polynomial: computed once per shape, read-only"""
    key = (d, n, l, seed)
    if key not in _encoded:
        coeffs = rand_ints(d, 7000 * d + n + l if seed is None else seed)
        ys, proofs = k.KZG.new().encode_cosets(coeff_form(k, coeffs), srs, n, l)
        ys.setflags(write=False)
        proofs.setflags(write=False)
        _encoded[key] = (coeffs, ys, proofs)
    return _encoded[key]


@pytest.mark.parametrize("d,n,l", SHAPES)
def test_rows_equal_the_encoder(k, ref_srs, d, n, l):
    coeffs, want_ys, want_proofs = encoded(k, ref_srs, d, n, l)
    m = n // l
    kzg = k.KZG.new()
    poly = coeff_form(k, coeffs)
    # every coset, shuffled (k = 0: c = 1 and k = m / 2: c = -1 among them)
    every = list(range(m))
    random.Random(d + n + l).shuffle(every)
    ys, proofs = kzg.prove_cosets(poly, ref_srs, n, every, l)
    assert ys.shape == (m, l, 4) and ys.dtype == np.uint64 and proofs.shape == (m, 8) and proofs.dtype == np.uint64
    assert np.array_equal(ys, want_ys[every]) and np.array_equal(proofs, want_proofs[every])
    # a single item
    for one in (0, m // 2, m - 1):
        ys1, proofs1 = kzg.prove_cosets(poly, ref_srs, n, [one], l)
        assert np.array_equal(ys1, want_ys[[one]]) and np.array_equal(proofs1, want_proofs[[one]]), one
    # duplicates
    dup = [0, m // 2, 0, m - 1, m // 2, 1 % m, 0]
    ys_d, proofs_d = kzg.prove_cosets(poly, ref_srs, n, dup, l)
    assert np.array_equal(ys_d, want_ys[dup]) and np.array_equal(proofs_d, want_proofs[dup])
    # eval form: the d evaluations on the d-point domain
    ys_e, proofs_e = kzg.prove_cosets(k.PolynomialEvalForm(pyref.frs_to_mont(pyref.dft(coeffs))), ref_srs, n, dup, l)
    assert np.array_equal(ys_e, ys_d) and np.array_equal(proofs_e, proofs_d)
    # each output alone: the same bits, nothing written for the one left out
    data = pyref.frs_to_mont(coeffs)
    rc, ys_v, out_v, inf_v, _ = raw_prove(k, ref_srs, data, 1, d, 0, n, l, None, dup, proofs=False)
    assert rc == 0 and np.array_equal(ys_v, ys_d) and np.all(out_v == 7) and np.all(inf_v == 7)
    rc, ys_p, out_p, inf_p, _ = raw_prove(k, ref_srs, data, 1, d, 0, n, l, None, dup, values=False)
    assert rc == 0 and np.array_equal(out_p, proofs_d) and np.all(ys_p == 7)
    assert np.array_equal(inf_p, (~np.asarray(proofs_d).any(axis=1)).astype(np.uint8))
    assert kzg.prove_cosets(poly, ref_srs, n, dup, l, values=False)[0] is None and kzg.prove_cosets(poly, ref_srs, n, dup, l, proofs=False)[1] is None


# ---- 2. larger chains: several segments, more than one carry level ---------------------------------------------------------------------
@pytest.mark.parametrize("l", [1, 64])
def test_larger_chains(k, big_srs, l):
    d, n = 1 << 14, 1 << 15
    coeffs, want_ys, want_proofs = encoded(k, big_srs, d, n, l)
    m = n // l
    items = [0, m // 2] + random.Random(l).sample(range(m), 38)
    ys, proofs = k.KZG.new().prove_cosets(coeff_form(k, coeffs), big_srs, n, items, l)
    assert np.array_equal(ys, want_ys[items]) and np.array_equal(proofs, want_proofs[items])


def test_the_tested_shapes_reach_every_kind_of_chain(k):
    info = k.helpers.prove_cosets_info
    one = info(64, 128, 1, 5)                       # D = 64 = S: one segment, no carry
    assert (one["seg_len"], one["segments"], one["carry_levels"]) == (64, 1, 0)
    tiny = info(64, 512, 32, 5)                     # D = 2: S = 2
    assert (tiny["seg_len"], tiny["segments"], tiny["carry_levels"]) == (2, 1, 0)
    several = info(2048, 4096, 1, 5)                # D = 2048: 32 segments, their heads one segment
    assert (several["seg_len"], several["segments"], several["carry_levels"]) == (64, 32, 1)
    deep = info(1 << 14, 1 << 15, 1, 40)            # D = 2^14: 256 segments (more than 64), two carry levels
    assert (deep["seg_len"], deep["segments"], deep["carry_levels"]) == (64, 256, 2)
    mid = info(1 << 14, 1 << 15, 64, 40)            # D = 256: 4 segments
    assert (mid["segments"], mid["carry_levels"]) == (4, 1)
    assert info(2048, 4096, 1, 1)["msm_single"] in (True, False) and not info(2048, 4096, 1, 2)["msm_single"]
    assert info(2048, 4096, 1, 4096)["items_per_group"] == 4096 and info(2048, 4096, 1, 4096, group_bytes=1)["items_per_group"] == 1


# ---- 3. the quotients themselves ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", [1, 16])
def test_quotients_equal_the_synthetic_division(k, l):
    d, n = 2048, 4096
    m = n // l
    coeffs = rand_ints(d, 300 + l)
    w = pyref.root_of_unity(12)
    items = [0, m // 2, 1, m - 1, 777 % m]
    q, ys = k.KZG.new().coset_quotients(coeff_form(k, coeffs), n, None, items, l, values=True)
    assert q.shape == (len(items), d, 4) and ys.shape == (len(items), l, 4)
    for i, kk in enumerate(items):
        want_q, want_r = div_xl(coeffs, l, pow(w, kk * l, R_))
        assert np.array_equal(q[i, :d - l], pyref.frs_to_mont(want_q)), kk
        assert not q[i, d - l:].any(), kk                               # the top l words of the row are zero
        for j in range(l):                                              # r reproduces the values
            assert np.array_equal(ys[i, j], pyref.fr_to_mont(pyref.poly_eval(want_r, pow(w, kk + j * m, R_)))), (kk, j)
    only_q, none = k.KZG.new().coset_quotients(coeff_form(k, coeffs), n, None, items, l)
    assert none is None and np.array_equal(only_q, q)


# ---- 4. degenerate polynomials -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", [1, 4])
def test_degenerate_polynomials(k, ref_srs, l):
    d, n = 64, 128
    m = n // l
    items = [0, m // 2, 3, m - 1]
    for coeffs in ([0] * d, [12345] + [0] * (d - 1)):                   # zero; only f_0: identity proofs, constant values
        rc, ys, out, inf, _ = raw_prove(k, ref_srs, pyref.frs_to_mont(coeffs), 1, d, 0, n, l, None, items)
        assert rc == 0 and not out.any() and np.all(inf == 1)
        assert np.array_equal(ys, np.broadcast_to(np.asarray(pyref.fr_to_mont(coeffs[0]), dtype=np.uint64), (len(items), l, 4)))
    half = rand_ints(d // 2, 41) + [0] * (d // 2)                       # the top half zero
    want_ys, want_proofs = k.KZG.new().encode_cosets(coeff_form(k, half), ref_srs, n, l)
    rc, ys, out, inf, _ = raw_prove(k, ref_srs, pyref.frs_to_mont(half), 1, d, 0, n, l, None, items)
    assert rc == 0 and np.array_equal(ys, want_ys[items]) and np.array_equal(out, want_proofs[items]) and not inf.any()


# ---- 5. several polynomials, several groups ---------------------------------------------------------------------------------------------
def test_several_polynomials_and_groups(k, ref_srs):
    d, n, l = 256, 512, 16
    m = n // l
    kzg = k.KZG.new()
    polys = [rand_ints(d, 500 + b) for b in range(3)]
    enc = [kzg.encode_cosets(coeff_form(k, p), ref_srs, n, l) for p in polys]
    rnd = random.Random(51)
    ps = [2, 0, 2, 0, 0, 2, 2, 0, 0, 2, 0]                              # mixed, polynomial 1 unreferenced
    ks = [0, m // 2] + [rnd.randrange(m) for _ in range(len(ps) - 2)]
    want_ys = np.stack([enc[b][0][c] for b, c in zip(ps, ks)])
    want_proofs = np.stack([enc[b][1][c] for b, c in zip(ps, ks)])
    forms = [coeff_form(k, p) for p in polys]
    ys, proofs = kzg.prove_cosets_batch(forms, ref_srs, n, ps, ks, l)
    assert np.array_equal(ys, want_ys) and np.array_equal(proofs, want_proofs)
    forms[1] = coeff_form(k, rand_ints(d, 599))                         # an unreferenced polynomial changes nothing
    ys2, proofs2 = kzg.prove_cosets_batch(forms, ref_srs, n, ps, ks, l)
    assert np.array_equal(ys2, ys) and np.array_equal(proofs2, proofs)
    all3 = [1, 2, 0, 1, 1, 0]                                           # every polynomial, eval form, as one array
    arr = np.stack([np.asarray(pyref.frs_to_mont(pyref.dft(p)), dtype=np.uint64).reshape(d, 4) for p in polys])
    ys3, proofs3 = kzg.prove_cosets_batch(arr, ref_srs, n, all3, ks[:6], l, eval_form=True)
    assert np.array_equal(ys3, np.stack([enc[b][0][c] for b, c in zip(all3, ks[:6])]))
    assert np.array_equal(proofs3, np.stack([enc[b][1][c] for b, c in zip(all3, ks[:6])]))
    # a budget small enough for >= 3 groups: the same bits
    ctx = ref_srs.ctx
    item_bytes = k.helpers.prove_cosets_info(d, n, l, len(ps), count=3)["item_bytes"]
    budget = 4 * item_bytes
    assert k.helpers.prove_cosets_info(d, n, l, len(ps), count=3, group_bytes=budget)["groups"] >= 3
    ctx.set_encode_group_bytes(budget)
    try:
        ys4, proofs4 = kzg.prove_cosets_batch(forms, ref_srs, n, ps, ks, l)
        ctx.set_encode_group_bytes(1)                                   # groups of one item
        ys5, proofs5 = kzg.prove_cosets_batch(forms, ref_srs, n, ps, ks, l)
    finally:
        ctx.set_encode_group_bytes(0)
    assert np.array_equal(ys4, ys) and np.array_equal(proofs4, proofs) and np.array_equal(ys5, ys) and np.array_equal(proofs5, proofs)


# ---- 6. the protocol round trip ----------------------------------------------------------------------------------------------------------
def test_recover_then_reseed_the_missing_cosets(k):
    d, n, l = 256, 512, 16
    m = n // l
    rnd = random.Random(61)
    poly = coeff_form(k, [rnd.randrange(R_) for _ in range(d)])
    srs = k.SRS.generate(TAU, d)
    kzg = k.KZG.new()
    commitment = kzg.commit_coeff_form(poly, srs)
    ys, proofs = kzg.encode_cosets(poly, srs, n, l)
    lost = sorted(rnd.sample(range(m), 5))
    present = [c for c in range(m) if c not in lost]
    got = kzg.recover_from_cosets(present, np.ascontiguousarray(ys[present]), n, degree_bound=d, eval_form=False)
    recovered = k.PolynomialCoeffForm(np.ascontiguousarray(got.coeffs()[:d]))
    ys5, proofs5 = kzg.prove_cosets(recovered, srs, n, lost, l)
    assert np.array_equal(ys5, ys[lost]) and np.array_equal(proofs5, proofs[lost])
    g2 = k.helpers.g2_mul_generator(k.fr.fr_from_int(pow(TAU, l, R_)))
    assert k.verifier.verify_multiproof_batch([commitment], [0] * 5, lost, ys5, list(proofs5), n, srs, g2) is True
    bad = ys5.copy()
    bad[3, 7] = pyref.fr_to_mont(pyref.fr_from_mont(bad[3, 7]) + 1)     # one value changed
    assert k.verifier.verify_multiproof_batch([commitment], [0] * 5, lost, bad, list(proofs5), n, srs, g2) is False
    srs.close()


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------
def test_error_table_in_its_order(k, ref_srs, test_srs_wire):
    L = k._lib
    lib = L.load()
    ctx = ref_srs.ctx
    coeffs, want_ys, want_proofs = encoded(k, ref_srs, 64, 128, 1)
    good = np.ascontiguousarray(pyref.frs_to_mont(coeffs), dtype=np.uint64)

    def still_works():                                                  # the context is usable after each error
        rc, ys, out, inf, _ = raw_prove(k, ref_srs, good, 1, 64, 0, 128, 1, None, [5, 64])
        assert rc == 0 and np.array_equal(ys, want_ys[[5, 64]]) and np.array_equal(out, want_proofs[[5, 64]])

    big = np.zeros((3 << 12, 4), dtype=np.uint64)
    ys = np.full((8, 64, 4), 7, dtype=np.uint64)
    out = np.full((8, 8), 7, dtype=np.uint64)
    inf = np.full(8, 7, dtype=np.uint8)
    ks = np.array([0, 1, 2, 3], dtype=np.uint64)
    ps = np.array([0, 0, 0, 0], dtype=np.uint64)
    bad = C.c_uint64(99)
    lag = ref_srs.lagrange(64)
    other_ctx = L.Context(0)
    other_srs = k.SRS(test_srs_wire[:64], order=64, ctx=other_ctx)
    NOARG = object()

    def call(srs_h, d, n, l, count=1, data=big, ctx_h=ctx.handle, ks_p=NOARG, ps_p=None, ni=4, ys_p=NOARG, out_p=NOARG, inf_p=NOARG):
        rc = lib.kzg_prove_cosets(ctx_h, srs_h, None if data is None else L.ptr(data), count, d, 0, n, l, ps_p, L.ptr(ks) if ks_p is NOARG else ks_p, ni,
                                  L.ptr(ys) if ys_p is NOARG else ys_p, L.ptr(out) if out_p is NOARG else out_p,
                                  inf.ctypes.data_as(L.u8p) if inf_p is NOARG else inf_p, C.byref(bad))
        if rc != 0:
            still_works()
        return rc

    h = ref_srs.handle
    # 1. null pointers, no output, proofs without flags, count = 0 -- in front of a length that is no power of two
    assert call(h, 3, 0, 1, ctx_h=None) == L.ERR_INVALID_ARG
    assert call(None, 3, 0, 1) == L.ERR_INVALID_ARG
    assert call(h, 3, 0, 1, data=None) == L.ERR_INVALID_ARG
    assert call(h, 3, 0, 1, ks_p=None) == L.ERR_INVALID_ARG
    assert call(h, 3, 0, 1, ys_p=None, out_p=None) == L.ERR_INVALID_ARG
    assert call(h, 3, 0, 1, inf_p=None) == L.ERR_INVALID_ARG
    assert call(h, 3, 0, 1, count=0) == L.ERR_INVALID_ARG
    # 2. an SRS of another context, a Lagrange-basis handle -- in front of the same
    assert call(other_srs.handle, 3, 0, 1) == L.ERR_INVALID_ARG
    assert call(lag.handle, 3, 0, 1) == L.ERR_INVALID_ARG
    # 3. the encoder's rows 3 .. 6 with their codes, each in front of the next
    assert call(h, 0, 64, 1) == L.ERR_NOT_POWER_OF_TWO
    assert call(h, 48, 1 << 25, 1) == L.ERR_NOT_POWER_OF_TWO
    assert call(h, 64, 96, 1) == L.ERR_NOT_POWER_OF_TWO
    assert call(h, 1, 1 << 25, 3) == L.ERR_DOMAIN
    assert call(h, 4096, 2048, 1) == L.ERR_INVALID_ARG                  # poly_len > n
    assert call(h, 1, 64, 1) == L.ERR_INVALID_ARG                       # poly_len = 1
    assert call(h, 4096, 4096, 3) == L.ERR_INVALID_ARG                  # l not a power of two
    assert call(h, 64, 4096, 64) == L.ERR_INVALID_ARG                   # l > poly_len / 2
    ks[2] = 1 << 40                                                     # (a bad item behind a capacity error is not looked at)
    assert call(h, 4096, 4096, 1) == L.ERR_SRS_CAPACITY_EXCEEDED and bad.value == 99
    # 4. the items: the smallest bad one is named
    ks[:] = [0, 127, 128, 500]
    assert call(h, 64, 128, 1) == L.ERR_INVALID_ARG and bad.value == 2
    ks[:] = [0, 127, 3, 5]
    ps[:] = [0, 2, 0, 3]
    bad.value = 99
    assert call(h, 64, 128, 1, count=2, ps_p=L.ptr(ps)) == L.ERR_INVALID_ARG and bad.value == 1
    ps[:] = [0, 1, 0, 1]
    ks[:] = [0, 31, 3, 32]                                              # m = 128 / 4 = 32
    assert call(h, 64, 128, 4, count=2, ps_p=L.ptr(ps)) == L.ERR_INVALID_ARG and bad.value == 3
    ks[:] = [0, 1, 2, 3]
    # 5. sizes that overflow size_t (an n_items that large has no index array to go with it: the query below takes that row)
    assert call(h, 64, 128, 1, count=(1 << 64) // (64 * 32) + 1) == L.ERR_INVALID_ARG
    assert np.all(ys == 7) and np.all(out == 7) and np.all(inf == 7)    # no output touched
    # n_items = 0: nothing written; flags are not needed for values alone
    assert call(h, 64, 128, 1, ni=0) == 0 and np.all(ys == 7) and np.all(out == 7) and np.all(inf == 7)
    assert call(h, 64, 128, 1, data=good, out_p=None, inf_p=None) == 0
    assert np.array_equal(ys.reshape(-1, 4)[:4], want_ys[:4, 0]) and np.all(ys.reshape(-1, 4)[4:] == 7) and np.all(out == 7)
    # the quotients' entry: no SRS, the same order
    qs = np.full((4, 64, 4), 7, dtype=np.uint64)
    cq = lambda d, n, l, count=1, data=big, q_p=L.ptr(qs), ni=4: lib.kzg_coset_quotients(
        ctx.handle, None if data is None else L.ptr(data), count, d, 0, n, l, None, L.ptr(ks), ni, q_p, None, C.byref(bad))
    assert cq(3, 0, 1, q_p=None) == L.ERR_INVALID_ARG and cq(3, 0, 1, data=None) == L.ERR_INVALID_ARG and cq(3, 0, 1, count=0) == L.ERR_INVALID_ARG
    assert cq(64, 96, 1) == L.ERR_NOT_POWER_OF_TWO and cq(1, 1 << 25, 3) == L.ERR_DOMAIN and cq(64, 4096, 64) == L.ERR_INVALID_ARG
    ks[1] = 128
    assert cq(64, 128, 1) == L.ERR_INVALID_ARG and bad.value == 1
    ks[1] = 1
    assert cq(64, 128, 1, count=(1 << 64) // (64 * 32) + 1) == L.ERR_INVALID_ARG and np.all(qs == 7)
    assert cq(64, 128, 1, data=good) == 0 and not np.all(qs == 7)
    still_works()
    # while a kzg_*_begin is in flight on slot 0 the call is refused; after its end it runs
    sc = np.ascontiguousarray(pyref.frs_to_mont(rand_ints(64, 71)), dtype=np.uint64)
    assert lib.kzg_msm_g1_srs_begin(ctx.handle, h, 0, L.ptr(sc), 64, 0) == 0
    refused = lib.kzg_prove_cosets(ctx.handle, h, L.ptr(good), 1, 64, 0, 128, 1, None, L.ptr(ks), 1, L.ptr(ys), None, None, C.byref(bad))
    pt = np.zeros(8, dtype=np.uint64)
    assert lib.kzg_msm_g1_srs_end(ctx.handle, 0, L.ptr(pt), None, None) == 0
    assert refused == L.ERR_INVALID_ARG and "in flight" in ctx.last_error()
    still_works()
    # the pure query keeps rows 3 .. 5 and check 5
    info = L.ProveCosetsInfo()
    q = lambda d, n, l, count=1, ni=4, v=1, p=1, out_p=C.byref(info): lib.kzg_prove_cosets_info(d, n, l, count, ni, v, p, 0, out_p)
    assert q(64, 128, 1, out_p=None) == L.ERR_INVALID_ARG and q(64, 128, 1, v=0, p=0) == L.ERR_INVALID_ARG and q(64, 128, 1, count=0) == L.ERR_INVALID_ARG
    assert q(64, 96, 1) == L.ERR_NOT_POWER_OF_TWO and q(1, 1 << 25, 3) == L.ERR_DOMAIN and q(64, 4096, 64) == L.ERR_INVALID_ARG
    assert q(1 << 14, 1 << 14, 1) == 0 and q(64, 128, 1, ni=(1 << 64) // 64 + 1) == L.ERR_INVALID_ARG
    # the Python surface: the argument errors mirror encode_cosets
    kzg = k.KZG.new()
    poly = coeff_form(k, coeffs)
    with pytest.raises(k.errors.GenericError):
        kzg.prove_cosets(poly, ref_srs, 256, [0], 3)
    with pytest.raises(k.errors.GenericError):
        kzg.prove_cosets(poly, ref_srs, 256, [0], 64)
    with pytest.raises(k.errors.FFTError):
        kzg.prove_cosets(poly, ref_srs, 96, [0], 1)
    with pytest.raises(k.errors.SrsCapacityExceeded):
        kzg.prove_cosets(k.PolynomialCoeffForm(big[:4096]), ref_srs, 4096, [0], 1)
    with pytest.raises(k.errors.GenericError):
        kzg.prove_cosets(poly, ref_srs, 128, [128], 1)
    with pytest.raises(k.errors.GenericError):
        kzg.prove_cosets_batch([poly], ref_srs, 128, [1], [0], 1)
    with pytest.raises(k.errors.GenericError):
        kzg.prove_cosets(poly, ref_srs, 128, [0], 1, values=False, proofs=False)
    with pytest.raises(TypeError):
        kzg.prove_cosets(good, ref_srs, 128, [0], 1)
    with pytest.raises(ValueError):                                     # KZG_ERR_INVALID_ARG, as everywhere in the library
        kzg.prove_cosets(poly, lag, 128, [0], 1)
    ys0, proofs0 = kzg.prove_cosets(poly, ref_srs, 128, [], 1)
    assert ys0.shape == (0, 1, 4) and proofs0.shape == (0, 8)
    still_works()
    lag.close()
    other_srs.close()
    other_ctx.close()


# ---- 8. the bound-checked build runs the comparisons with every site counter at 0 ------------------------------------------------------
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
WORKLOAD = ["tests/test_gpu_prove_cosets.py::" + t for t in ("test_rows_equal_the_encoder", "test_degenerate_polynomials", "test_several_polynomials_and_groups")]


def test_bound_checked_build_keeps_every_precondition():
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": WORKLOAD}], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "PYTEST_RC 0" in out, (out[-3000:], res.stderr[-2000:])
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert sites
    fired = {int(s[1]): int(s[2]) for s in sites if int(s[2])}
    assert not fired, fired
