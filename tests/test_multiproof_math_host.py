"""CPU-only checks of the FK20 multi-proofs (`kzg_compute_multiproofs`): the algorithm's indexing restated over Fr with a known tau
against the direct quotient, the coset layout of the chunks, the C-ABI declarations of the three new entries, and the argument errors
the Python surface raises before it touches a device."""
import os
import random
import re

import numpy as np
import pytest

import pyref
from pyref import R_, dft, poly_eval, root_of_unity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("kzg_compute_multiproofs", "kzg_srs_cache_multiproof", "kzg_srs_drop_multiproof")


def div_xl(f, l, c):
    """f = q (X^l - c) + r"""
    f = list(f)
    q = [0] * max(len(f) - l, 0)
    for i in range(len(f) - 1, l - 1, -1):
        co = f[i]
        q[i - l] = co
        f[i] = 0
        f[i - l] = (f[i - l] + co * c) % R_
    return q, f[:l]


def fk20(f, l, tau):
    """The device pipeline over Fr, tau known: [tau^i]_1 -> tau^i, G1 FFTs -> Fr DFTs (natural order, library roots)."""
    n = len(f)
    m = n // l
    H = [0] * (2 * m)
    for b in range(l):
        F = [f[j * l + b] for j in range(m)] + [0] * m                        # F^(b)
        S = [pow(tau, (m - 2 - t) * l + b, R_) for t in range(m - 1)] + [0] * (m + 1)   # S^(b)
        Fh, Sh = dft(F), dft(S)
        H = [(H[t] + Fh[t] * Sh[t]) % R_ for t in range(2 * m)]
    hh = dft(H, inverse=True)
    h = hh[m - 1:2 * m - 1]
    assert h[m - 1] == 0
    return dft(h)                                                              # root w^l = the library's m-th root


@pytest.mark.parametrize("log_n", range(1, 7))
def test_fk20_indexing_matches_the_direct_quotient(log_n):
    n = 1 << log_n
    rnd = random.Random(log_n)
    tau = rnd.randrange(R_)
    f = [rnd.randrange(R_) for _ in range(n)]
    w = root_of_unity(log_n)
    f_tau = poly_eval(f, tau)
    l = 1
    while l <= n // 2:
        m = n // l
        assert pow(w, l, R_) == root_of_unity(log_n - (l.bit_length() - 1))
        pi = fk20(f, l, tau)
        for k in range(m):
            c = pow(w, k * l, R_)
            q, r = div_xl(f, l, c)
            assert pi[k] == poly_eval(q, tau) == (f_tau - poly_eval(r, tau)) * pow((pow(tau, l, R_) - c) % R_, -1, R_) % R_, (n, l, k)
            if l == 1:                                                         # the one-point proof at z = w^k
                assert pi[k] == (f_tau - poly_eval(f, c)) * pow((tau - c) % R_, -1, R_) % R_
        l *= 2


@pytest.mark.parametrize("n,l", [(8, 2), (16, 4), (32, 8), (64, 4)])
def test_chunk_k_is_the_coset_of_indices_k_plus_jm(n, l):
    rnd = random.Random(n + l)
    f = [rnd.randrange(R_) for _ in range(n)]
    w = root_of_unity(n.bit_length() - 1)
    evals = dft(f)
    m = n // l
    for k in range(m):
        c = pow(w, k * l, R_)
        _, r = div_xl(f, l, c)
        for j in range(l):
            x = pow(w, k + j * m, R_)
            assert pow(x, l, R_) == c                                          # the coset's points are the roots of X^l - w^(k l)
            assert evals[k + j * m] == poly_eval(f, x) == poly_eval(r, x)


def test_header_declares_the_three_entries_as_the_prototypes_do():
    import rust_kzg_bn254_amd as k
    hdr = open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in k._lib.PROTOTYPES, name
    u64p, u8p, vp, sz, i32 = k._lib.u64p, k._lib.u8p, k._lib.vp, k._lib.sz, k._lib.i32
    assert k._lib.PROTOTYPES["kzg_compute_multiproofs"] == (i32, [vp, vp, u64p, sz, i32, sz, u64p, u8p])
    assert k._lib.PROTOTYPES["kzg_srs_cache_multiproof"] == (i32, [vp, vp, sz, sz])
    assert k._lib.PROTOTYPES["kzg_srs_drop_multiproof"] == (i32, [vp, vp])


def test_library_exports_the_three_entries():
    import ctypes as C
    import rust_kzg_bn254_amd as k
    lib = C.CDLL(k._lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name


class _FakeSrs:
    def __init__(self, n):
        self._n = n

    def __len__(self):
        return self._n


def test_python_argument_errors_need_no_device():
    import rust_kzg_bn254_amd as k
    kzg = k.KZG.new()                                                          # no context is created before the arguments pass
    poly = k.PolynomialCoeffForm(pyref.frs_to_mont(list(range(1, 65))))
    srs = _FakeSrs(64)
    for bad in (0, -2, 3, 12):
        with pytest.raises(k.errors.GenericError, match="power of 2"):
            kzg.compute_multiproofs(poly, srs, bad)
    with pytest.raises(k.errors.GenericError, match="half"):
        kzg.compute_multiproofs(poly, srs, 64)
    with pytest.raises(k.errors.GenericError):
        kzg.compute_multiproofs(k.PolynomialCoeffForm(pyref.frs_to_mont([5])), srs, 1)
    with pytest.raises(k.errors.SrsCapacityExceeded):
        kzg.compute_multiproofs(poly, _FakeSrs(32), 1)
    with pytest.raises(TypeError):
        kzg.compute_multiproofs(np.zeros((64, 4), np.uint64), srs, 1)
    assert kzg.ctx is None
