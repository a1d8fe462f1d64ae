"""-m gpu: kzg_g1_ifft at the sizes where its stage plan (csrc/g1fft_plan.h) changes form, on known-tau SRSs: 1 point (no stage) and 2 (one
K = 1 stage), each also on a copy of the first n points as an SRS of its own (no per-bit tables); either side of the per-bit-table
thresholds 32 | 64, 256 | 512, 2 048 | 4 096; 2^13 (seven pair stages, the last of radix 2), 2^16 (radix-2 butterflies on pairs) and 2^17
(radix-2 butterflies on lanes, the form of every larger size).  Every checked output against L_i = l_i(tau) G by big-integer arithmetic:
all of them up to 128 points, indices 0, 1, 2, n - 1 and a few in between above."""
import numpy as np
import pytest

import pyref
from pyref import R_

pytestmark = pytest.mark.gpu

TAU = int.from_bytes(__import__("hashlib").sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % R_


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


@pytest.fixture(scope="module")
def srs15(k):
    s = k.SRS.generate(TAU, 1 << 15)
    yield s
    s.close()


@pytest.fixture(scope="module")
def srs17(k):
    s = k.SRS.generate(TAU, 1 << 17)
    yield s
    s.close()


def check_lagrange_basis(L, n):
    """L_i = l_i(tau) G with l_i(tau) = (tau^n - 1) / n . w^i / (tau - w^i) (the closed form of test_g1_ifft_through_the_per_bit_tables)"""
    assert len(L) == n
    log_n = n.bit_length() - 1
    w = pyref.root_of_unity(log_n)
    zn = (pow(TAU, n, R_) - 1) * pow(n, -1, R_) % R_
    if n <= 128:
        indices = range(n)
    else:
        indices = sorted({0, 1, 2, n // 4 - 1, n // 2, n // 2 + 1, 3 * n // 4 + 5, n - 2, n - 1})
    for i in indices:
        wi = pow(w, i, R_)
        li = zn * wi % R_ * pow(TAU - wi, -1, R_) % R_
        assert pyref.point_from_wire(L[i]) == pyref.ec_mul(li, (1, 2)), (n, i)


@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_points(k, srs15, n):
    kzg = k.KZG.new()
    L = kzg.g1_ifft(n, srs15)
    check_lagrange_basis(L, n)
    small = k.SRS(np.ascontiguousarray(srs15.g1[:n]), order=n)
    try:
        check_lagrange_basis(kzg.g1_ifft(n, small), n)
    finally:
        small.close()


@pytest.mark.parametrize("n", [32, 64, 256, 512, 2048, 4096])
def test_either_side_of_the_per_bit_table_thresholds(k, srs15, n):
    check_lagrange_basis(k.KZG.new().g1_ifft(n, srs15), n)


@pytest.mark.parametrize("log_n", [13, 16, 17])
def test_pair_stages_with_a_radix_2_tail_and_radix_2_butterflies(k, srs17, log_n):
    check_lagrange_basis(k.KZG.new().g1_ifft(1 << log_n, srs17), 1 << log_n)
