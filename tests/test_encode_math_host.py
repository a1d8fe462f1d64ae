"""CPU-only checks of the encoder (`kzg_encode_cosets`): its five steps restated over Fr with a known tau against the direct quotients
of the zero-padded polynomial, the spread load of the radix-2 form followed by the stages it leaves against the full transform of the
padded vector, the coset-major layout of the values, the C-ABI declaration, and the argument errors the Python surface raises before it
touches a device."""
import os
import random
import re

import numpy as np
import pytest

import pyref
from pyref import R_, dft, poly_eval, root_of_unity
from test_multiproof_math_host import _FakeSrs, div_xl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def radix2_stages(x, first, w, last=None):
    """k_g1fft_stage over Fr: decimation in time, in place, on bit-reversed input; the stages first .. last (log2 len(x)); w the len(x)-th root"""
    x = list(x)
    n = len(x)
    log_n = n.bit_length() - 1
    for s in range(first, (log_n if last is None else last) + 1):
        half = 1 << (s - 1)
        for b in range(n // 2):
            j = b & (half - 1)
            i0 = ((b >> (s - 1)) << s) | j
            i1 = i0 + half
            t = x[i1] * pow(w, j << (log_n - s), R_) % R_
            x[i0], x[i1] = (x[i0] + t) % R_, (x[i0] - t) % R_
    return x


def spread_load(h, log_m):
    """planes[i] = h[bitrev_{log2 m'}(i >> log2 r)], i < m: the bit reversal and the stages 1 .. log2 r of the input h zero-padded to m"""
    log_nz = len(h).bit_length() - 1
    log_r = log_m - log_nz
    return [h[bitrev(i >> log_r, log_nz)] for i in range(1 << log_m)], log_r


def encode(f, n, l, tau, pruned):
    """The device pipeline over Fr, tau known: steps 1-4 see d = len(f) only, step 5 is the m-point transform of h zero-padded."""
    d = len(f)
    m, mp = n // l, d // l
    M = 2 * mp
    H = [0] * M
    for b in range(l):
        F = [f[j * l + b] for j in range(mp)] + [0] * mp
        S = [pow(tau, (mp - 2 - t) * l + b, R_) for t in range(mp - 1)] + [0] * (mp + 1)
        Fh, Sh = dft(F), dft(S)
        H = [(H[t] + Fh[t] * Sh[t]) % R_ for t in range(M)]
    h = dft(H, inverse=True)[mp - 1:2 * mp - 1]
    assert h[mp - 1] == 0
    log_m = m.bit_length() - 1
    if not pruned:
        return dft(h + [0] * (m - mp))                                         # the m-th root is w^l
    x, log_r = spread_load(h, log_m)
    return radix2_stages(x, log_r + 1, root_of_unity(log_m))


@pytest.mark.parametrize("d,n,l", [(16, 64, 2), (8, 8, 1), (32, 256, 4), (16, 32, 1), (2, 64, 1), (16, 128, 8)])
def test_the_five_steps_match_the_direct_quotients(d, n, l):
    rnd = random.Random(d * 1000 + n + l)
    tau = rnd.randrange(R_)
    f = [rnd.randrange(R_) for _ in range(d)]
    w = root_of_unity(n.bit_length() - 1)
    m = n // l
    pi = encode(f, n, l, tau, pruned=False)
    assert pi == encode(f, n, l, tau, pruned=True)                             # the pruned transform equals the full one
    f_tau = poly_eval(f, tau)
    for k in range(m):
        c = pow(w, k * l, R_)
        q, r = div_xl(f, l, c)
        assert len(q) == d - l                                                 # degree < d - l: tau^0 .. tau^(d - l - 1) suffice
        assert pi[k] == poly_eval(q, tau) == (f_tau - poly_eval(r, tau)) * pow((pow(tau, l, R_) - c) % R_, -1, R_) % R_, (d, n, l, k)


@pytest.mark.parametrize("log_m,log_nz", [(1, 1), (2, 1), (5, 1), (5, 3), (5, 4), (5, 5), (7, 2)])
def test_spread_load_then_the_remaining_stages_is_the_dft_of_the_padded_vector(log_m, log_nz):
    rnd = random.Random(log_m * 16 + log_nz)
    h = [rnd.randrange(R_) for _ in range(1 << log_nz)]
    m = 1 << log_m
    padded = h + [0] * (m - len(h))
    w = root_of_unity(log_m)
    x, log_r = spread_load(h, log_m)
    assert log_r == log_m - log_nz
    # the load IS the bit-reversed padded vector after its stages 1 .. log2 r
    assert x == radix2_stages([padded[bitrev(i, log_m)] for i in range(m)], 1, w, last=log_r)
    assert radix2_stages(x, log_r + 1, w) == dft(padded)


@pytest.mark.parametrize("d,n,l", [(4, 8, 2), (8, 32, 4), (16, 16, 1), (2, 16, 1)])
def test_values_are_coset_major_rows_of_the_padded_dft(d, n, l):
    import rust_kzg_bn254_amd as k
    rnd = random.Random(d + n + l)
    f = [rnd.randrange(R_) for _ in range(d)]
    evals = dft(f + [0] * (n - d))
    m, r = n // l, n // d
    ys = [[evals[k_ + j * m] for j in range(l)] for k_ in range(m)]            # ys[k][j] = evals[k + j m]: the kernel's index rule
    flat = [v for row in ys for v in row]
    assert all(flat[i] == evals[(i // l) + (i % l) * m] for i in range(n))
    want = k.KZG.new().cosets(k.PolynomialEvalForm(pyref.frs_to_mont(evals)), l)
    assert np.array_equal(np.asarray(pyref.frs_to_mont(flat), dtype=np.uint64).reshape(m, l, 4), want)
    assert [evals[i * r] for i in range(d)] == dft(f)                          # the d-point domain is every r-th point of the n-point one


def test_header_declares_the_entry_as_the_prototype_does():
    import ctypes as C
    import rust_kzg_bn254_amd as k
    hdr = open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read()
    mt = re.search(r"int32_t\s+kzg_encode_cosets\s*\(([^;]*)\);", hdr)
    assert mt, "kzg_encode_cosets is not declared"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", mt.group(1), flags=re.S).split(",")]
    assert [re.sub(r"\s+\w+$", "", a) for a in args] == ["kzg_ctx*", "kzg_srs*", "const uint64_t*", "size_t", "int32_t", "size_t", "size_t", "uint64_t*", "uint64_t*",
                                                         "uint8_t*"]
    u64p, u8p, vp, sz, i32 = k._lib.u64p, k._lib.u8p, k._lib.vp, k._lib.sz, k._lib.i32
    assert k._lib.PROTOTYPES["kzg_encode_cosets"] == (i32, [vp, vp, u64p, sz, i32, sz, sz, u64p, u64p, u8p])
    assert hasattr(C.CDLL(k._lib.LIB_PATH), "kzg_encode_cosets")


def test_python_argument_errors_need_no_device():
    import rust_kzg_bn254_amd as k
    kzg = k.KZG.new()                                                          # no context is created before the arguments pass
    poly = k.PolynomialCoeffForm(pyref.frs_to_mont(list(range(1, 65))))
    srs = _FakeSrs(64)
    for bad in (0, -2, 3, 12):
        with pytest.raises(k.errors.GenericError, match="power of 2"):
            kzg.encode_cosets(poly, srs, 256, bad)
    with pytest.raises(k.errors.GenericError, match="half"):
        kzg.encode_cosets(poly, srs, 256, 64)                                  # l <= d / 2, not n / 2
    with pytest.raises(k.errors.GenericError):
        kzg.encode_cosets(k.PolynomialCoeffForm(pyref.frs_to_mont([5])), srs, 4, 1)
    with pytest.raises(k.errors.GenericError):
        kzg.encode_cosets(poly, srs, 32, 1)                                    # n < d
    with pytest.raises(k.errors.GenericError):
        kzg.encode_cosets(poly, srs, 256, 1, values=False, proofs=False)
    for bad_n in (0, 96, 255):
        with pytest.raises(k.errors.FFTError):
            kzg.encode_cosets(poly, srs, bad_n, 1)
    with pytest.raises(k.errors.FFTError):
        kzg.encode_cosets(poly, srs, 1 << 25, 1)
    with pytest.raises(k.errors.SrsCapacityExceeded):
        kzg.encode_cosets(poly, _FakeSrs(63), 256, 1)
    with pytest.raises(TypeError):
        kzg.encode_cosets(np.zeros((64, 4), np.uint64), srs, 256, 1)
    assert kzg.ctx is None
