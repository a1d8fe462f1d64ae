"""CPU: the property k_msm_accumulate's loop relies on since it adds with the UNCHECKED mixed addition (csrc/curve.h xyzz_madd<.., false>):

    the ZZ of a sum of mixed additions that started from an affine point is == 0 mod p  <=>  one of the additions met P == +-Q,

so one fe_is_zero_mod(acc.zz) per finished partial sum replaces the test per entry, and a sum that did not meet such a pair is limb for
limb the sum the checked addition gives.  tests/hostcheck/replaycheck.cpp compiles the same headers with g++ and -DKZG_BOUND_CHECK (every
lazy-reduction bound aborts, also on the meaningless values a tainted sum goes on with) and runs both forms over the same entries;
the checked sum is compared with big integers (tests/pyref.py).  All points are small multiples of the generator."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pyref
from pyref import P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
SRC = os.path.join(HERE, "hostcheck", "replaycheck.cpp")
SO = os.path.join(HERE, "hostcheck", "libreplaycheck.so")
G = (1, 2)
u32p = C.POINTER(C.c_uint32)
i32p = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def rc():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("field29.h", "curve.h", "field_constants.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DKZG_BOUND_CHECK", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-I" + CSRC, "-o", SO, SRC])
    lib = C.CDLL(SO)
    lib.kzg_rc_chain.restype = None
    lib.kzg_rc_chain.argtypes = [u32p, u32p, C.c_uint32, u32p, i32p, u32p, i32p, u32p, u32p]
    return lib


_MULT = {}


def mult(s):
    if s not in _MULT:
        _MULT[s] = pyref.ec_mul(s, G) if s else None
    return _MULT[s]


def chain(rc, entries):
    """entries: (s, neg): add (neg ? -1 : 1) * s G.  -> (tainted, unchecked limbs, unchecked inf, checked limbs, checked inf, checked affine point)"""
    n = len(entries)
    pts = np.ascontiguousarray(pyref.points_to_wire([mult(s) for s, _ in entries])).view(np.uint32).reshape(-1)
    neg = np.array([g for _, g in entries], dtype=np.uint32)
    tainted = C.c_uint32(0); iu = C.c_uint32(0); ic = C.c_uint32(0)
    lu = np.zeros(36, np.int32); lc = np.zeros(36, np.int32); wire = np.zeros(32, np.uint32)
    rc.kzg_rc_chain(pts.ctypes.data_as(u32p), neg.ctypes.data_as(u32p), n, C.byref(tainted), lu.ctypes.data_as(i32p), C.byref(iu),
                    lc.ctypes.data_as(i32p), C.byref(ic), wire.ctypes.data_as(u32p))
    w = wire.view(np.uint64).reshape(4, 4)
    if ic.value:
        pt = None
    else:
        x, y, zz, zzz = (pyref.fq_from_mont(w[q]) for q in range(4))
        pt = (x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P)
    return bool(tainted.value), lu, bool(iu.value), lc, bool(ic.value), pt


def expected(entries):
    return mult_sum(sum((-s if g else s) for s, g in entries))


def mult_sum(v):
    from pyref import R_
    v %= R_
    return pyref.ec_mul(v, G) if v else None


def meets_exception(entries):
    """Does the running sum of the (checked) chain ever equal +- the next point?  Running sums as multiples of G."""
    acc = None                                # None: identity
    for s, g in entries:
        if s == 0:
            continue
        v = -s if g else s
        if acc is not None and acc in (v, -v):
            return True
        acc = v if acc is None else acc + v
        if acc == 0:
            acc = None
    return False


def test_sums_without_an_exceptional_pair_are_limb_identical_and_untainted(rc):
    rnd = random.Random(1)
    ran = 0
    for _ in range(200):
        entries = [(rnd.randrange(0, 60), rnd.randrange(2)) for _ in range(rnd.randrange(1, 12))]
        if meets_exception(entries):
            continue
        ran += 1
        tainted, lu, iu, lc, ic, pt = chain(rc, entries)
        assert not tainted, entries
        assert iu == ic and np.array_equal(lu, lc), entries
        assert pt == expected(entries), entries
    assert ran > 100


@pytest.mark.parametrize("head", [[(1, 0), (1, 0)], [(1, 0), (1, 1)], [(5, 1), (5, 1)], [(2, 0), (3, 0), (5, 0)], [(2, 0), (3, 0), (5, 1)],
                                  [(7, 0), (0, 0), (7, 0)], [(4, 1), (1, 0), (3, 0), (9, 0), (9, 1)]],
                         ids=["G+G", "G-G", "-5G-5G", "2G+3G+5G", "2G+3G-5G", "7G+O+7G", "sum to O, then 9G-9G"])
def test_an_exceptional_pair_taints_the_sum_and_the_taint_stays(rc, head):
    """P + P and P - P at the start of a sum, behind ordinary additions and behind an identity entry; then up to ten further entries,
    among them the points that would cancel the meaningless running value: ZZ stays == 0 mod p, no bound is exceeded, and the checked
    form over the same entries is the big-integer sum."""
    rnd = random.Random(len(head))
    assert meets_exception(head)
    for tail_len in range(0, 11):
        for _ in range(6):
            entries = head + [(rnd.randrange(0, 30), rnd.randrange(2)) for _ in range(tail_len)]
            tainted, lu, iu, lc, ic, pt = chain(rc, entries)
            assert tainted and not iu, entries
            assert pt == expected(entries), entries
            assert ic == (pt is None)


def test_a_single_entry_and_an_empty_sum_are_untainted(rc):
    for entries in ([(3, 0)], [(3, 1)], [(0, 0)], [(0, 0), (0, 1)]):
        tainted, lu, iu, lc, ic, pt = chain(rc, entries)
        assert not tainted and iu == ic and np.array_equal(lu, lc)
        assert pt == expected(entries)
    tainted, lu, iu, lc, ic, pt = chain(rc, [(0, 0)])
    assert iu and not lu.any(), "the identity flag comes with literally zero limbs"
