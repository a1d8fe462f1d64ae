"""CPU: the preconditions of the field layer (csrc/field29.h) and the generated products (csrc/fe_asm.h).

* fe_asm.h is exactly what tools/gen_fe_asm.py emits (no hand edit, no drift between the generator and the header the device runs).
* Every bound predicate of field29.h fires on an operand just outside its bound and stays quiet just inside (a checker that has never
  fired is no evidence): the predicates are evaluated through libhostcheck.so without aborting.
* Every operand set of tests/fe_operands.py -- the ones test_gpu_device_math.py sends to the device -- passes the bound-checked host
  build (an illegal operand aborts there) and gives the big-integer value and output range the header states.
"""
import ctypes as C
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

import fe_operands as F
from test_field29_host import CSRC, ROOT, hc  # noqa: F401  (the module fixture that builds libhostcheck.so)

i32p = C.POINTER(C.c_int32)

# site numbers: enum KzgBoundSite of field29.h
(MUL_LIMBS, MUL_VALUE, MULSUB_LIMBS, MULSUB_VALUE, IS_ZERO_MOD, CANON, REDUCE, REDUCE_SMALL, TO_WIRE, PACK, ADD, SUB, DBL, NORM) = range(14)


def test_fe_asm_header_is_what_the_generator_emits(tmp_path):
    out = tmp_path / "fe_asm.h"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_fe_asm.py"), "--out", str(out)], stdout=subprocess.DEVNULL, timeout=120)
    assert filecmp.cmp(str(out), os.path.join(CSRC, "fe_asm.h"), shallow=False), "csrc/fe_asm.h differs from tools/gen_fe_asm.py's output"
    text = out.read_text()
    for name in ("FE_ASM_INSTRUCTIONS_SQR", "FE_ASM_INSTRUCTIONS_MUL2", "FE_ASM_INSTRUCTIONS_SQR2", "FE_ASM_INSTRUCTIONS_MULSUB", "FE_ASM_INSTRUCTIONS_MUL"):
        assert name in text


def _pred(hc, which, site, *ops):
    buf = np.array(F.row(*ops), dtype=np.int64)
    assert buf.min() >= -(1 << 31) and buf.max() < (1 << 31)
    buf = buf.astype(np.int32)
    hc.hc_predicate.restype = C.c_int
    r = hc.hc_predicate(which, site, buf.ctypes.data_as(i32p))
    assert r in (0, 1), (site, r)
    return r


def _scaled(v, f):
    """an integer near f v, f a float close to 1 (relative spacing far above the 2^-50 of the C predicates' doubles)"""
    return v + int((f - 1.0) * 1e12) * (v // 10 ** 12)


def _controls(m):
    """(site, operands just inside, operands just outside) for every bound predicate"""
    L = F.limbs
    T = F.RADIX * m
    z = [0] * 9
    a0 = 10 ** 9
    b_in, b_out = int(F.MUL_LIMB_LIMIT / a0) - 1, int(F.MUL_LIMB_LIMIT / a0) + 2
    A = 1 << 257
    s_lim = F.MULSUB_LIMB_LIMIT
    c0 = 1 << 29
    d_in, d_out = int(s_lim * (1 - 1e-9)) // c0, int(s_lim * (1 + 1e-9)) // c0
    big = (1 << 31) - 1
    red = F.REDUCE_LIMIT * m
    cases = [
        (MUL_LIMBS, ([a0] + z[1:], [b_in] + z[1:]), ([a0] + z[1:], [b_out] + z[1:])),
        (MUL_LIMBS, ([0] * 8 + [a0], [0] * 8 + [b_in]), ([0] * 3 + [-a0] + [0] * 5, [0] * 8 + [-b_out])),
        (MUL_VALUE, (L(A), L(_scaled(T // A, 1 - 1e-9))), (L(A), L(_scaled(T // A, 1 + 1e-9)))),
        (MUL_VALUE, (L(-A), L(_scaled(T // A, 1 - 1e-9))), (L(-A), L(-_scaled(T // A, 1 + 1e-9)))),
        (MULSUB_LIMBS, ([1] + z[1:], [1] + z[1:], [c0] + z[1:], [d_in] + z[1:]), ([1] + z[1:], [1] + z[1:], [c0] + z[1:], [d_out] + z[1:])),
        (MULSUB_VALUE, (L(A), L(_scaled(T // A // 2, 1 - 1e-9)), L(-A), L(_scaled(T // A // 2, 1 - 1e-9))),
                       (L(A), L(_scaled(T // A // 2, 1 + 1e-9)), L(-A), L(_scaled(T // A // 2, 1 + 1e-9)))),
    ]
    for site in (IS_ZERO_MOD, CANON):
        cases += [(site, (L(2 * m - 1),), (L(2 * m),)), (site, (L(-m + 1),), (L(-m),)),
                  (site, (L(5),), ([5 + (1 << 29), -1] + z[2:],))]              # same value, not normalised
    for site in (REDUCE, REDUCE_SMALL):
        cases += [(site, (L(_scaled(red, 1 - 1e-9)),), (L(_scaled(red, 1 + 1e-9)),)),
                  (site, (L(-_scaled(red, 1 - 1e-9)),), (L(-_scaled(red, 1 + 1e-9)),)),
                  (site, ([big - 3, 0] + z[2:],), ([big, big] + z[2:],))]        # the normalisation's carry overflows limb 1
    cases += [(TO_WIRE, (L(_scaled(red, 1 - 1e-9)),), (L(_scaled(red, 1 + 1e-9)),)), (TO_WIRE, (L(7),), ([7 + (1 << 29), -1] + z[2:],)),
              (PACK, (L((1 << 256) - 1),), (L(1 << 256),)), (PACK, (L(0),), (L(-1),)), (PACK, (L(3),), ([-1, 1] + z[2:],)),
              (ADD, ([big - 5] * 9, [5] * 9), ([big - 5] * 9, [6] + [5] * 8)), (ADD, ([-(1 << 31) + 5] * 9, [-5] * 9), ([-(1 << 31) + 5] * 9, [-5] * 8 + [-6])),
              (SUB, ([-(1 << 31) + 5] * 9, [5] * 9), ([-(1 << 31) + 5] * 9, [5] * 4 + [6] + [5] * 4)), (SUB, ([big - 5] * 9, [-5] * 9), ([big - 5] * 9, [-6] * 9)),
              (DBL, ([(1 << 30) - 1] * 9,), ([(1 << 30) - 1] * 8 + [1 << 30],)), (DBL, ([-(1 << 30)] * 9,), ([-(1 << 30) - 1] + [0] * 8,)),
              (NORM, ([-(1 << 31) + 4] * 8 + [0],), ([-(1 << 31)] * 8 + [0],)), (NORM, ([big, big - 3] + [0] * 7,), ([big, big - 2] + [0] * 7,))]
    return cases


@pytest.mark.parametrize("which", [0, 1])
def test_every_bound_predicate_fires_just_outside_and_stays_quiet_just_inside(hc, which):  # noqa: F811
    m = F.MODS[which]
    hc.hc_sites.restype = C.c_int
    assert hc.hc_sites() == 14
    seen = set()
    for site, inside, outside in _controls(m):
        assert _pred(hc, which, site, *inside) == 1, ("quiet inside", site, inside)
        assert _pred(hc, which, site, *outside) == 0, ("fires outside", site, outside)
        seen.add(site)
    assert seen == set(range(14))


def _host_run(hc, op, which, rows):
    out = np.zeros((rows.shape[0], 18), np.int32)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    hc.hc_prim(which, op, rows.ctypes.data_as(i32p), out.ctypes.data_as(i32p), C.c_size_t(rows.shape[0]))
    return out


@pytest.mark.parametrize("op", range(len(F.NAMES)), ids=F.NAMES)
def test_operand_sets_are_legal_and_the_host_form_gives_the_stated_values(hc, op):  # noqa: F811
    """The host (g++, KZG_BOUND_CHECK) third of the device conformance comparison: every edge row and a random sample, both fields."""
    for which in (0, 1):
        edges = F.edge_rows(op, which)
        rand = F.random_rows(op, which, 4096)
        rows = np.concatenate([edges, rand])
        out = _host_run(hc, op, which, rows)                  # aborts on any operand outside a precondition
        bad = F.check_values(op, which, rows, out, np.arange(rows.shape[0]))
        assert not bad, bad[:3]


def test_operand_sets_reach_the_bounds(hc):  # noqa: F811
    """The saturating sets really saturate: limb products and values within 1 % of fe_mul's, fe_sqr's and fe_mulsub's limits, both at
    once in some rows, and fe_sqr's doubled limb at ~2^30.7."""
    for which in (0, 1):
        m = F.MODS[which]
        T = F.RADIX * m
        e = F.edge_rows(F.MUL, which)
        lim = [F.max_limb(r[0:9]) * F.max_limb(r[9:18]) / F.MUL_LIMB_LIMIT for r in e.tolist()]
        val = [abs(F.value(r[0:9]) * F.value(r[9:18])) / T for r in e.tolist()]
        assert max(lim) < 1 and max(val) < 1
        assert sum(x >= 0.99 for x in lim) >= 300 and sum(v >= 0.99 for v in val) >= 300
        assert sum(x >= 0.99 and v >= 0.99 for x, v in zip(lim, val)) >= 100
        s = F.edge_rows(F.SQR, which)
        assert max(2 * F.max_limb(r[0:9]) for r in s.tolist()) > 2 ** 30.6
        q = F.edge_rows(F.MULSUB, which).tolist()
        ql = [(F.max_limb(r[0:9]) * F.max_limb(r[9:18]) + F.max_limb(r[18:27]) * F.max_limb(r[27:36])) / F.MULSUB_LIMB_LIMIT for r in q]
        qv = [(abs(F.value(r[0:9]) * F.value(r[9:18])) + abs(F.value(r[18:27]) * F.value(r[27:36]))) / T for r in q]
        assert sum(x >= 0.99 for x in ql) >= 300 and sum(v >= 0.99 for v in qv) >= 300
        assert sum(x >= 0.99 and v >= 0.99 for x, v in zip(ql, qv)) >= 100


def test_reduce_small_of_a_negative_value_may_end_just_below_zero(hc):  # noqa: F811
    """Finding of these tests: for a negative input fe_reduce_small's quotient over-estimates a / m, so the result can be slightly
    negative (field29.h once stated [0, 1.0001 m)).  The NTT's last pass follows it with fe_canon, whose range (-m, 2m) covers it."""
    for which in (0, 1):
        m = F.MODS[which]
        rows = F.to_array([F.row(F.limbs(-k * m - 1)) for k in (1, 2, 6, 168)] + [F.row(F.limbs(-(168 * m) - (1 << 200)))])
        out = _host_run(hc, F.REDUCE_SMALL, which, rows)
        got = F.values(out)
        assert got[:3] == [-1, -1, -1]
        assert all(-m < 10000 * g < 0 for g in got)
        canon = _host_run(hc, F.CANON, which, np.concatenate([out[:, :9], np.zeros((len(got), 27), np.int32)], axis=1))
        assert F.values(canon) == [v % m for v in F.values(rows)]


def test_point_formulas_and_naf_rows_of_the_device_check_on_the_host(hc, test_srs_points):  # noqa: F811
    """The host third of the device checks of curve.h and naf.h (dc_curve / dc_naf of tests/devcheck/dc_prims.h), bound-checked:
    every formula including its exceptional cases equals the affine group law, every NAF row reproduces its scalar."""
    import random
    rnd = random.Random(5)
    cases = F.curve_cases(test_srs_points, rnd, 60)
    rows = F.curve_rows(cases)
    u32p = C.POINTER(C.c_uint32)
    for op in (F.MADD, F.PADD, F.PDBL):
        out = np.zeros((len(cases), 32), np.uint32)
        hc.hc_curve(op, rows.ctypes.data_as(u32p), out.ctypes.data_as(u32p), C.c_size_t(len(cases)))
        for i, (p1, p2, s) in enumerate(cases):
            assert F.xyzz_wire_to_affine(out[i]) == F.curve_expected(op, p1, p2, s), (F.CURVE_NAMES[op], i)
    ks, scal, width = F.naf_rows(rnd, 100)
    out = np.zeros((len(width), 64), np.uint32)
    hc.hc_naf_rows(scal.ctypes.data_as(u32p), width.ctypes.data_as(i32p), out.ctypes.data_as(u32p), C.c_size_t(len(width)))
    for i in range(len(width)):
        assert F.naf_value(out[i], int(width[i])) == ks[i // len(F.NAF_WIDTHS)], i
