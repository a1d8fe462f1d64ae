"""-m gpu: the GLV decomposition and the three GLV scalar multiplications on the device, at their edges.

glv_decompose (csrc/glv.h) against the plain-integer restatement of tests/glv_ref.py, word for word, on the scalars where the halves
come closest to the 127 bits the chains read.  xyzz_scalar_mul (one lane), pair_scalar_mul (two lanes) and quad_scalar_mul (four
lanes, csrc/glv_lanes.h) on the SAME rows, each result compared as an affine group element with pyref.ec_mul of the value the
halves stand for.  The halves are given directly, so the rows reach what no decomposed scalar does: a positive second half, a large
negative first half, and -- through the lattice vectors (a1, b1), (a2, b2), which sum to 0 mod r -- the doubling and cancellation
branches inside the chains from a base that is not the identity.  pair_madd / pair_add / pair_dbl and their quad forms run on the
exceptional rows of the one-lane formula test.  Everything runs once more through the bound-check build, whose counters must stay
at zero.  Rows are tiled so that every case sits at many lane positions and next to ordinary rows.  Values are compared; nothing
here hunts for a fault.
"""
import ctypes as C
import random

import numpy as np
import pytest

import fe_operands as F
import glv_ref as G
import pyref
from pyref import R_
from test_gpu_device_math import _first_diff, _tile, dc  # noqa: F401  (module fixture: libdevcheck.so)

pytestmark = pytest.mark.gpu

u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
i32p = C.POINTER(C.c_int32)
FORMS = ("lane", "pair", "quad")
N_GLV = 1 << 15
N_SMUL = 1 << 13
N_CURVE = 1 << 14


def _ptr(a):
    return a.ctypes.data_as(u32p)


def run_glv(dc, prefix, k_rows):  # noqa: F811
    out = np.zeros_like(k_rows)
    rc = getattr(dc, prefix + "glv")(_ptr(k_rows), _ptr(out), C.c_uint32(k_rows.shape[0]))
    assert rc == 0, (prefix, rc)
    return out


def run_smul(dc, prefix, form, rows):  # noqa: F811
    out = np.zeros((rows.shape[0], 32), np.uint32)
    rc = getattr(dc, prefix + "smul")(form, _ptr(rows), _ptr(out), C.c_uint32(rows.shape[0]))
    assert rc == 0, (prefix, FORMS[form], rc)
    return out


def run_lanes_curve(dc, prefix, form, op, rows):  # noqa: F811
    out = np.zeros((rows.shape[0], 32), np.uint32)
    rc = getattr(dc, prefix + "lanes_curve")(form, op, _ptr(rows), _ptr(out), C.c_uint32(rows.shape[0]))
    assert rc == 0, (prefix, FORMS[form], F.CURVE_NAMES[op], rc)
    return out


def words(k):
    return [(k >> (32 * j)) & 0xFFFFFFFF for j in range(8)]


def halves_words(m1, s1, m2, s2):
    """magnitudes below 2^127 and explicit sign bits (a zero half may carry either sign) -> the eight words of the chains' contract"""
    assert 0 <= m1 < G.HALF and 0 <= m2 < G.HALF
    w = words(m1 | (m2 << 128))
    w[3] |= s1 << 31
    w[7] |= s2 << 31
    return w


# ----- decomposition --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def glv_scalars():
    ks = G.scalars()
    if len(ks) % 2 == 0:                     # an odd count: every repeat of the tiling puts a scalar on another lane
        ks = ks + [ks[-1] ^ 1]
    return ks, np.array([words(k) for k in ks], np.uint32), np.array([G.decompose(k) for k in ks], np.uint32)


def test_device_glv_decompose_matches_the_restatement(dc, glv_scalars):  # noqa: F811
    ks, k_rows, want = glv_scalars
    assert len(ks) >= 2400 and G.K2_EXTREME in ks
    rows, want_t = _tile(k_rows, N_GLV), _tile(want, N_GLV)
    for prefix in ("dc_asm_", "dc_cpp_"):
        got = run_glv(dc, prefix, rows)
        assert np.array_equal(got, want_t), (prefix, _first_diff(got, want_t, rows))


# ----- scalar multiplication --------------------------------------------------------------------------------------------------------
def smul_halves(rnd):
    """[(label, m1, s1, m2, s2)]: every pair of halves of the test, inside the contract (magnitudes below 2^127)"""
    top = G.HALF - 1
    p01, p10, p0011 = int("01" * 64, 2) & top, int("10" * 64, 2) & top, int("0011" * 32, 2) & top
    p1100 = int("1100" * 32, 2) & top
    h = [("zero", 0, 0, 0, 0)]
    for s1 in (0, 1):
        for s2 in (0, 1):
            h += [("one,0", 1, s1, 0, s2), ("0,one", 0, s1, 1, s2), ("top,top", top, s1, top, s2)]
    h += [("bit126,0", 1 << 126, 0, 0, 0), ("0,bit126", 0, 0, 1 << 126, 1), ("bit126,bit0", 1 << 126, 1, 1, 0), ("bit0,bit126", 1, 0, 1 << 126, 0),
          ("bit126,bit126", 1 << 126, 0, 1 << 126, 0)]
    pats = (p01, p10, p0011)
    for a in pats:                           # every value of the quad form's 2-bit window pair, a zero window after a non-zero one
        for b in pats:
            h.append(("pattern", a, rnd.randrange(2), b, rnd.randrange(2)))
    h += [("pattern", p0011, 0, p1100, 1), ("pattern", p1100, 1, p0011, 0)]
    for s in (0, 1):
        h += [("random,0", rnd.randrange(G.HALF), s, 0, 0), ("0,random", 0, 0, rnd.randrange(G.HALF), s)]
    for bits in (1, 7, 13, 19):              # the accumulator stays at the identity for more than 100 steps
        h.append(("short", rnd.randrange(1 << (bits - 1), 1 << bits), rnd.randrange(2), rnd.randrange(1 << bits), rnd.randrange(2)))
    h += [("short", 0, 0, rnd.randrange(1 << 18, 1 << 19), 1), ("short", rnd.randrange(1 << 18, 1 << 19), 1, 0, 0)]
    for _ in range(100):
        h.append(("random", rnd.randrange(G.HALF), rnd.randrange(2), rnd.randrange(G.HALF), rnd.randrange(2)))
    groups = G.scalar_groups()
    dec = groups["extremes"] + groups["edges"] + groups["floor_boundaries"][:20] + groups["lambda_multiples"][:5] + groups["random"][:14]
    assert len(dec) == 60
    for k in dec:
        k1, k2 = G.split(k)
        h.append(("decomposed", abs(k1), int(k1 < 0), abs(k2), int(k2 < 0)))
    # the lattice rows: the exceptional branches from a base that is not the identity
    a1, a2, b1m, b2 = G.A1, G.A2, G.B1M, G.B2
    for flip in (0, 1):
        h += [("lattice a1,b1 (0: cancels)", a1, flip, b1m, 1 - flip), ("lattice a2,b2 (0: cancels, k2 > 0)", a2, flip, b2, flip),
              ("lattice a1+2,b1 (2: doubles P1)", a1 + 2, flip, b1m, 1 - flip), ("lattice a2+2,b2+2 (2+2 lambda: doubles S)", a2 + 2, flip, b2 + 2, flip)]
    return h


@pytest.fixture(scope="module")
def smul_cases(test_srs_points):
    """(labels, rows n x 40, expected affine points): every pair of halves on an affine base, a P1 + P2 base (stored form, ZZ != 1) and the
    identity base (P1 = -P2), shuffled so that every wave of the tiling mixes them.  Expected points are computed here, once."""
    rnd = random.Random(127)
    pts = test_srs_points
    labels, rows, want = [], [], []
    for label, m1, s1, m2, s2 in smul_halves(rnd):
        kk = halves_words(m1, s1, m2, s2)
        value = G.halves_value(kk)
        assert value == ((-m1 if s1 else m1) + (-m2 if s2 else m2) * G.LAMBDA) % R_
        q, a, b = (pts[rnd.randrange(len(pts))] for _ in range(3))
        for kind, p1, p2 in (("affine", None, q), ("sum", a, b), ("identity", pyref.ec_neg(q), q)):
            base = pyref.ec_add(p1, p2)
            assert (base is None) == (kind == "identity")
            labels.append((label, kind))
            rows.append(list(pyref.point_to_wire(p1).view(np.uint32)) + list(pyref.point_to_wire(p2).view(np.uint32)) + kk)
            want.append(pyref.ec_mul(value, base))
    for (label, kind), w in zip(labels, want):      # the lattice rows do what they are there for
        if kind != "identity" and label.startswith("lattice") and "cancels" in label:
            assert w is None
    order = list(range(len(rows)))
    rnd.shuffle(order)
    if len(order) % 2 == 0:                  # an odd count: every repeat of the tiling puts a row on another lane, pair and quad
        order.append(order[0])
    return [labels[i] for i in order], np.array([rows[i] for i in order], np.uint32), [want[i] for i in order]


def _check_smul(out, n, cases, who):
    labels, _, want = cases
    for i in range(n):
        got = F.xyzz_wire_to_affine(out[i])
        assert got == want[i], (who, i, labels[i], got, want[i])


@pytest.mark.parametrize("form", range(3), ids=FORMS)
def test_device_glv_scalar_mul_is_the_group_law(dc, smul_cases, form):  # noqa: F811
    labels, base, want = smul_cases
    d = base.shape[0]
    assert 400 <= d <= 800 and d % 2 == 1
    rows = _tile(base, N_SMUL)
    got = run_smul(dc, "dc_asm_", form, rows)
    _check_smul(got, d, smul_cases, FORMS[form])
    # the same row gives the same words wherever it sits in a wave
    again = _tile(got[:d], N_SMUL)
    assert np.array_equal(got, again), (FORMS[form], "lane position changes the result", _first_diff(got, again, rows))
    cpp = run_smul(dc, "dc_cpp_", form, base)
    if form == 0:
        assert np.array_equal(cpp, got[:d]), ("device C++ != device asm", _first_diff(cpp, got[:d], base))
    else:
        _check_smul(cpp, d, smul_cases, FORMS[form] + " (C++ products)")


# ----- the point formulas of the lane forms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", range(3), ids=F.CURVE_NAMES)
def test_device_lane_form_point_formulas(dc, op, test_srs_points):  # noqa: F811
    """pair_madd / pair_add / pair_dbl(_any) and quad_madd / quad_add / quad_dbl(_any) == the affine group law on the rows of the one-lane
    formula test: random pairs, the same point, the negated point, the identity and -3 P2, at every position of a pair / quad in the wave."""
    cases = F.curve_cases(test_srs_points, random.Random(100 + op), 200)
    cases.append(cases[0])                   # an odd count, as above
    want = [F.curve_expected(op, p1, p2, s) for p1, p2, s in cases]
    base = F.curve_rows(cases)
    rows = _tile(base, N_CURVE)
    for form in (1, 2):
        got = run_lanes_curve(dc, "dc_asm_", form, op, rows)
        for i, w in enumerate(want):
            assert F.xyzz_wire_to_affine(got[i]) == w, (FORMS[form], F.CURVE_NAMES[op], i, cases[i])
        again = _tile(got[:len(cases)], N_CURVE)
        assert np.array_equal(got, again), (FORMS[form], F.CURVE_NAMES[op], _first_diff(got, again, rows))


# ----- the operand ranges inside the chains --------------------------------------------------------------------------------------------
def test_device_glv_bound_check_counters_stay_at_zero(dc, glv_scalars, smul_cases, test_srs_points):  # noqa: F811
    """The decomposition, scalar-multiplication and lane-form rows once through the KZG_DEVICE_BOUND_CHECK build: no lazy-reduction
    precondition of field29.h is violated inside the chains (the one-lane form's un-normalised +-Y, the (-7m, 5m) X of a stored base,
    the lanes whose product is not used).  The results are the group law's here too.  (Positive control: test_gpu_device_math.py.)
    This is the test that found xyzz_scalar_mul handing back +-P / +-phi(P) with limb-negated, un-normalised Y when the whole chain is one
    addition to the identity (halves (-1, 0), (0, -1)): right value, but not the stored form fe_to_wire and xyzz_store are promised."""
    dc.kzg_bc_read_devcheck.restype = C.c_int
    dc.kzg_bc_reset_devcheck.restype = C.c_int
    sites = 14
    counts = np.zeros(sites, np.uint64)
    first = np.zeros((sites, 9), np.int32)
    assert dc.kzg_bc_reset_devcheck() == 0
    _, k_rows, want = glv_scalars
    assert np.array_equal(run_glv(dc, "dc_bc_", k_rows), want)
    _, base, _ = smul_cases
    for form in range(3):
        _check_smul(run_smul(dc, "dc_bc_", form, base), base.shape[0], smul_cases, FORMS[form] + " (bound-check build)")
        assert dc.kzg_bc_read_devcheck(counts.ctypes.data_as(u64p), first.ctypes.data_as(i32p)) == 0
        assert not counts.any(), (FORMS[form], counts.tolist(), first.tolist())
    for op in range(3):
        cases = F.curve_cases(test_srs_points, random.Random(100 + op), 40)
        rows = F.curve_rows(cases)
        for form in (1, 2):
            got = run_lanes_curve(dc, "dc_bc_", form, op, rows)
            for i, (p1, p2, s) in enumerate(cases):
                assert F.xyzz_wire_to_affine(got[i]) == F.curve_expected(op, p1, p2, s), (FORMS[form], F.CURVE_NAMES[op], i)
            assert dc.kzg_bc_read_devcheck(counts.ctypes.data_as(u64p), first.ctypes.data_as(i32p)) == 0
            assert not counts.any(), (FORMS[form], F.CURVE_NAMES[op], counts.tolist(), first.tolist())
