"""CPU-only checks of erasure decoding (`kzg_recover_from_cosets`): the algorithm restated over Fr (tests/recover_ref.py) recovers
polynomials the test chose and flags inconsistent values, the C-ABI declaration and its prototype, and the argument errors the Python
surface raises before it touches a device."""
import os
import random
import re

import numpy as np
import pytest

import pyref
import recover_ref
from pyref import R_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 1, 4), (8, 4, 1), (16, 2, 5), (64, 4, 8), (2048, 16, 64), (2048, 1, 1024), (2048, 1024, 1)]     # (n, l, count)


def known_case(n, l, count, degree, seed):
    rnd = random.Random(seed)
    f = [rnd.randrange(R_) for _ in range(degree)] + [0] * (n - degree)
    ks = rnd.sample(range(n // l), count)
    return f, ks, recover_ref.coset_rows(recover_ref.fft(f), l, ks)


def test_fft_is_the_definition():
    vals = [random.Random(7).randrange(R_) for _ in range(16)]
    assert recover_ref.fft(vals) == pyref.dft(vals)
    assert recover_ref.fft(vals, inverse=True) == pyref.dft(vals, inverse=True)


@pytest.mark.parametrize("n,l,count", SHAPES)
def test_restatement_recovers_a_known_polynomial(n, l, count):
    f, ks, ys = known_case(n, l, count, count * l, n + l)
    got, consistent = recover_ref.recover(n, l, ks, ys)
    assert got == f and consistent


@pytest.mark.parametrize("n,l,count", [s for s in SHAPES if s[2] >= 2 and s[1] * s[2] >= 4 and s[0] <= 64])
def test_consistency_flag(n, l, count):
    d = count * l
    f, ks, ys = known_case(n, l, count, d // 2, 3 * n + l)
    got, consistent = recover_ref.recover(n, l, ks, ys, d // 2)
    assert got == f and consistent
    ys[0][0] = (ys[0][0] + 1) % R_                                            # one value changed
    got, consistent = recover_ref.recover(n, l, ks, ys, d // 2)
    assert not consistent and not any(got[d:])
    assert recover_ref.coset_rows(recover_ref.fft(got), l, ks) == ys           # still the interpolant of degree < count l
    assert recover_ref.recover(n, l, ks, ys)[1]                               # no bound: always consistent


def test_header_declares_the_entry_as_the_prototype_does():
    import rust_kzg_bn254_amd as k
    hdr = open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read()
    decl = re.search(r"int32_t\s+kzg_recover_from_cosets\s*\(([^;]*)\)\s*;", hdr)
    assert decl, "kzg_recover_from_cosets is not declared"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == 10, params
    assert [p.split()[-1] for p in params] == ["ctx", "ys_mont", "coset_indices", "count", "n", "chunk_len", "degree_bound", "eval_form",
                                               "out_poly_mont", "out_consistent"]
    L = k._lib
    assert L.PROTOTYPES["kzg_recover_from_cosets"] == (L.i32, [L.vp, L.u64p, L.u64p, L.sz, L.sz, L.sz, L.sz, L.i32, L.u64p, L.C.POINTER(L.i32)])


def test_library_exports_the_entry():
    import ctypes as C
    import rust_kzg_bn254_amd as k
    assert hasattr(C.CDLL(k._lib.LIB_PATH), "kzg_recover_from_cosets")


def test_python_argument_errors_need_no_device():
    import rust_kzg_bn254_amd as k
    kzg = k.KZG.new()                                                          # no context is created before the arguments pass
    G = k.errors.GenericError
    ys = np.zeros((2, 4, 4), dtype=np.uint64)
    with pytest.raises(G, match="shape"):
        kzg.recover_from_cosets([0, 1], np.zeros((2, 4), dtype=np.uint64), 16)
    with pytest.raises(G, match="shape"):
        kzg.recover_from_cosets([0, 1, 2], ys, 16)
    with pytest.raises(k.errors.FFTError):
        kzg.recover_from_cosets([0, 1], ys, 24)
    with pytest.raises(k.errors.FFTError):
        kzg.recover_from_cosets([0], np.zeros((1, 1, 4), dtype=np.uint64), 1)
    with pytest.raises(G, match="power of 2"):
        kzg.recover_from_cosets([0, 1], np.zeros((2, 3, 4), dtype=np.uint64), 16)
    with pytest.raises(G, match="half"):
        kzg.recover_from_cosets([0], np.zeros((1, 16, 4), dtype=np.uint64), 16)
    with pytest.raises(G, match="number of cosets"):
        kzg.recover_from_cosets([], np.zeros((0, 4, 4), dtype=np.uint64), 16)
    with pytest.raises(G, match="number of cosets"):
        kzg.recover_from_cosets(list(range(5)), np.zeros((5, 4, 4), dtype=np.uint64), 16)
    with pytest.raises(G, match="distinct"):
        kzg.recover_from_cosets([1, 1], ys, 16)
    with pytest.raises(G, match="distinct"):
        kzg.recover_from_cosets([0, 4], ys, 16)                                # m = 4
    with pytest.raises(G, match="too few"):
        kzg.recover_from_cosets([0, 1], ys, 16, degree_bound=9)
    assert kzg.ctx is None
