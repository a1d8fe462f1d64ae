"""The GLV constants and decomposition rule of csrc/glv.h in plain integers (tests/glv_ref.py reads the constants out of the header).

Checked here, without a GPU: the lattice and endomorphism identities, the rounding of g1 / g2, the magnitude bound the chains rely
on (they read exactly 127 bits of each half) derived from the constants with exact rationals, and on the scalar list of the device
test (tests/test_gpu_glv.py) that the halves recompose to the scalar and stay below 2^127.
"""
from fractions import Fraction

import glv_ref as G
import pyref
from pyref import P, R_

TWO256 = 1 << 256


def test_lattice_basis_and_cube_roots():
    assert G.B2 == G.A1
    assert G.A1 * G.B2 - G.A2 * (-G.B1M) == R_                   # a1 b2 - a2 b1 = r
    lam, beta = G.LAMBDA, G.BETA
    assert (G.A1 - G.B1M * lam) % R_ == 0 and (G.A2 + G.B2 * lam) % R_ == 0     # both basis vectors lie in {x + y lambda = 0 mod r}
    assert (lam * lam + lam + 1) % R_ == 0
    assert pow(beta, 3, P) == 1 and beta != 1 and 0 < beta < P


def test_endomorphism_is_multiplication_by_lambda(test_srs_points):
    for x, y in [pyref.G1, test_srs_points[1], test_srs_points[1234], test_srs_points[2999]]:
        assert pyref.on_curve((x, y))
        assert (G.BETA * x % P, y) == pyref.ec_mul(G.LAMBDA, (x, y))


def _round_div(a, b):
    return (2 * a + b) // (2 * b)


def test_g1_g2_are_the_rounded_quotients():
    assert G.G1 == _round_div(TWO256 * G.B2, R_)
    assert G.G2 == _round_div(TWO256 * G.B1M, R_)
    k = R_ - 1
    assert (k * G.G1) >> 256 < 1 << 64                             # c1 fits the two words glv_decompose keeps
    assert (k * G.G2) >> 256 < 1 << 128                            # c2 fits four


def derived_bounds():
    """(bound on |k1|, bound on |k2|) as exact rationals, from the header's constants alone.

    (k, 0) = x1 (a1, b1) + x2 (a2, b2) with x1 = k b2 / r, x2 = k |b1| / r (a1 b2 - a2 b1 = r).  c1 = floor(k g1 / 2^256), and
    k g1 / 2^256 is off x1 by at most e1 = r |g1 - 2^256 b2 / r| / 2^256 because k < r; so x1 - c1 lies in (-e1, 1 + e1), and x2 - c2
    in (-e2, 1 + e2) likewise.  Then k1 = (x1 - c1) a1 + (x2 - c2) a2 and k2 = -(x1 - c1) |b1| + (x2 - c2) b2.  In k2 the two terms have
    opposite signs when both differences are positive: its extreme is (1 + e1) |b1| from the first plus the e2 b2 the second adds on
    that side (the other side, e1 |b1| + (1 + e2) b2, is smaller by |b1| - b2)."""
    e1 = abs(G.G1 - Fraction(TWO256 * G.B2, R_)) * R_ / TWO256
    e2 = abs(G.G2 - Fraction(TWO256 * G.B1M, R_)) * R_ / TWO256
    assert e1 <= Fraction(1, 2) and e2 <= Fraction(1, 2)           # a rounded quotient is off by at most one half
    k1 = (1 + e1) * G.A1 + (1 + e2) * G.A2
    k2 = (1 + e1) * G.B1M + e2 * G.B2
    return k1, k2


def derived_k1_floor():
    """g2 is rounded up, so k g2 / 2^256 >= x2 and x2 - c2 > -e2; g1 is rounded down, so x1 - c1 >= 0: k1 > -e2 a2"""
    assert G.G1 * R_ < TWO256 * G.B2 and G.G2 * R_ > TWO256 * G.B1M
    return -(abs(G.G2 - Fraction(TWO256 * G.B1M, R_)) * R_ / TWO256) * G.A2


def test_halves_stay_below_2_127_for_every_canonical_scalar():
    k1, k2 = derived_bounds()
    print("derived bounds: |k1| <= %.8f 2^127, |k2| <= %.8f 2^127" % (float(k1 / G.HALF), float(k2 / G.HALF)))
    assert k1 < G.HALF
    assert k2 < G.HALF


def test_scalar_list_recomposes_and_respects_the_bounds():
    b1, b2 = derived_bounds()
    floor1 = derived_k1_floor()
    assert floor1 > -(2 ** 123.9)
    groups = G.scalar_groups()
    assert len(groups["random"]) == 2000 and len(groups["floor_boundaries"]) == 300
    big1 = big2 = 0
    for name, ks in groups.items():
        for k in ks:
            k1, k2 = G.split(k)
            kk = G.decompose(k)
            assert abs(k1) < G.HALF and abs(k2) < G.HALF, (name, hex(k))
            assert abs(k1) <= b1 and abs(k2) <= b2, (name, hex(k))
            assert G.unpack(kk) == (k1, k2), (name, hex(k))
            assert G.halves_value(kk) == k, (name, hex(k))
            # the sign facts stated in glv.h: the second half is never positive, the first never far below zero
            assert k2 <= 0 and k1 > -(2 ** 123.9) and k1 > floor1, (name, hex(k))
            big1, big2 = max(big1, abs(k1)), max(big2, abs(k2))
    print("largest on the list: |k1| = %.8f 2^127, |k2| = %.8f 2^127" % (big1 / G.HALF, big2 / G.HALF))
    # the list does reach the narrow end of the bound: the searched extremes are where the header's 6 % of headroom is measured
    assert abs(G.split(G.K2_EXTREME)[1]) > Fraction(94064745, 10 ** 8) * G.HALF
    assert big2 > Fraction(94, 100) * G.HALF and big1 > Fraction(8695, 10000) * G.HALF
    for k in groups["small"]:
        assert G.split(k) == (k, 0)                                # k < 2^64: c1 = c2 = 0


def test_restatement_matches_the_words_of_the_device_contract():
    assert G.decompose(0) == [0] * 8
    assert G.decompose(1) == [1, 0, 0, 0, 0, 0, 0, 0]
    assert G.pack(-1, -2) == [1, 0, 0, 1 << 31, 2, 0, 0, 1 << 31]
    assert G.halves_value(G.pack(-1, -2)) == (-1 - 2 * G.LAMBDA) % R_
    assert G.halves_value(G.pack(G.A1, -G.B1M)) == 0 and G.halves_value(G.pack(G.A2, G.B2)) == 0
