"""-m gpu: the field layer as it runs on the device, limb for limb.

tests/devcheck/devcheck.hip applies one primitive of tests/devcheck/dc_prims.h per lane over a full-chip launch, compiled as the
product compiles it (the generated inline-asm products of csrc/fe_asm.h) and with -DKZG_NO_FE_ASM (the C++ forms of field29.h on the
device).  Every result agrees three ways:
  1. limb for limb: device asm == device C++ == host C++ (libhostcheck.so, built with KZG_BOUND_CHECK, so every operand is also proven
     legal on the way);
  2. by value with big-integer arithmetic (a b 2^-261 mod m, ...) on the edge rows and a random sample (tests/fe_operands.py);
  3. inside the output range the header states for the primitive.
Operands (tests/fe_operands.py): extreme signed limb patterns, limb- and value-saturating products (each limit alone and both
together, fe_sqr's doubled limb at ~2^30.7, fe_mulsub at its column limit), canonical edges, the lazy ranges of curve.h and 2^20
random legal rows per product and field.  Every edge row sits at lanes 0, 31, 32 and 63 of several waves; the products run in four
launches, each with the rows rotated to other lanes and waves.  This compares values; it does not hunt for faults.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import fe_operands as F
from test_field29_host import hc  # noqa: F401  (module fixture: libhostcheck.so)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
DC = os.path.join(HERE, "devcheck")
SO = os.path.join(DC, "libdevcheck.so")
i32p = C.POINTER(C.c_int32)
u64p = C.POINTER(C.c_uint64)

N_PRODUCT = 1 << 20            # random legal rows per product per field
N_OTHER = 1 << 18             # (room for every edge row at four lanes of two waves)
N_BIGINT = 1 << 14             # rows checked by big-integer value per primitive and field (all edges + a random sample)
ROTATIONS = (0, 31, 32 * 64 + 33, 4099 * 64 + 17)   # the four launches of every product: rows shifted across lanes and waves

# (prefix, defines): the same source, three ways
VARIANTS = (("dc_asm_", []), ("dc_cpp_", ["-DKZG_NO_FE_ASM", "-DDC_PREFIX=dc_cpp_", "-DDC_NS=dc_cpp"]),
            ("dc_bc_", ["-DKZG_DEVICE_BOUND_CHECK", "-DDC_PREFIX=dc_bc_", "-DDC_NS=dc_bc"]))


def build_devcheck(out=SO):
    deps = [os.path.join(DC, f) for f in ("devcheck.hip", "dc_prims.h", "dc_glv.h")] + [os.path.join(CSRC, f) for f in
                                                                                         ("field29.h", "fe_asm.h", "fe_invert.h", "field_constants.h", "curve.h", "naf.h",
                                                                                          "curve_pair.h", "curve_quad.h", "glv.h", "glv_lanes.h")]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + CSRC]
    with tempfile.TemporaryDirectory() as tmp:
        objs, procs = [], []
        try:
            for prefix, defs in VARIANTS:
                objs.append(os.path.join(tmp, prefix + "devcheck.o"))
                procs.append(subprocess.Popen(["hipcc", *flags, *defs, "-c", os.path.join(DC, "devcheck.hip"), "-o", objs[-1]]))
            for p in procs:
                assert p.wait(timeout=900) == 0, "devcheck.hip does not compile"
        finally:
            for p in procs:                  # a failed or timed-out compile leaves no compiler behind
                if p.poll() is None:
                    p.kill()
                    p.wait()
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", os.path.join(tmp, "lib.so"), *objs], timeout=300)
        os.replace(os.path.join(tmp, "lib.so"), out)
    return out


@pytest.fixture(scope="module")
def dc():
    lib = C.CDLL(build_devcheck())
    for prefix, _ in VARIANTS:
        getattr(lib, prefix + "run").restype = C.c_int
        getattr(lib, prefix + "ops").restype = C.c_int
        getattr(lib, prefix + "curve").restype = C.c_int
        getattr(lib, prefix + "naf").restype = C.c_int
        getattr(lib, prefix + "glv").restype = C.c_int
        getattr(lib, prefix + "smul").restype = C.c_int
        getattr(lib, prefix + "lanes_curve").restype = C.c_int
        assert getattr(lib, prefix + "ops")() == len(F.NAMES)
    return lib


def device_run(dc, prefix, op, which, rows):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    out = np.zeros((rows.shape[0], 18), np.int32)
    rc = getattr(dc, prefix + "run")(which, op, rows.ctypes.data_as(i32p), out.ctypes.data_as(i32p), C.c_uint32(rows.shape[0]))
    assert rc == 0, f"{prefix}run({F.NAMES[op]}) returned HIP error {rc}"
    return out


def host_run(hc, op, which, rows):  # noqa: F811
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    out = np.zeros((rows.shape[0], 18), np.int32)
    hc.hc_prim(which, op, rows.ctypes.data_as(i32p), out.ctypes.data_as(i32p), C.c_size_t(rows.shape[0]))
    return out


def _first_diff(a, b, rows):
    i = int(np.nonzero((a != b).any(axis=1))[0][0])
    return {"row": i, "lane": i % 64, "wave": i // 64, "operands": rows[i].tolist(), "got": a[i].tolist(), "want": b[i].tolist()}


@pytest.mark.parametrize("op", range(len(F.NAMES)), ids=F.NAMES)
def test_device_primitive_three_ways(dc, hc, op):  # noqa: F811
    for which in (0, 1):
        edges = F.edge_rows(op, which)
        n = N_PRODUCT if op in F.PRODUCTS else N_OTHER
        rows, edge_idx = F.place(F.random_rows(op, which, n), edges, seed=op * 2 + which)
        host = host_run(hc, op, which, rows)
        # 2 + 3: value and range by big integers on every edge row and a random sample
        rng = np.random.default_rng(op)
        sample = np.unique(np.concatenate([edge_idx, rng.choice(n, size=max(0, N_BIGINT - edge_idx.size), replace=False)]))
        bad = F.check_values(op, which, rows, host, sample)
        assert not bad, ("host result off the big-integer value", bad[:2])
        # 1: device C++ and device asm limb for limb with the host
        cpp = device_run(dc, "dc_cpp_", op, which, rows)
        assert np.array_equal(cpp, host), ("device C++ != host", F.NAMES[op], which, _first_diff(cpp, host, rows))
        for rot in (ROTATIONS if op in F.PRODUCTS else ROTATIONS[:1]):
            rr = np.roll(rows, rot, axis=0)
            got = device_run(dc, "dc_asm_", op, which, rr)
            want = np.roll(host, rot, axis=0)
            assert np.array_equal(got, want), ("device asm != host", F.NAMES[op], which, rot, _first_diff(got, want, rr))


def test_device_bound_check_counters_fire_on_just_outside_operands(dc):
    """Positive control of the KZG_DEVICE_BOUND_CHECK build: one fe_mul operand pair just over the limb bound and one fe_is_zero_mod
    operand just outside (-m, 2m), each in one lane of a launch of legal rows.  The counters of exactly those sites fire once and keep
    the operand; the legal rows fire nothing.  (The illegal lanes give a wrong value; nothing faults.)"""
    dc.kzg_bc_read_devcheck.restype = C.c_int
    dc.kzg_bc_reset_devcheck.restype = C.c_int
    sites = 14
    counts = np.zeros(sites, np.uint64)
    first = np.zeros((sites, 9), np.int32)

    def read():
        assert dc.kzg_bc_read_devcheck(counts.ctypes.data_as(u64p), first.ctypes.data_as(i32p)) == 0
        return counts.copy(), first.copy()

    for which in (0, 1):
        m = F.MODS[which]
        assert dc.kzg_bc_reset_devcheck() == 0
        legal = F.random_rows(F.MUL, which, 4096)
        device_run(dc, "dc_bc_", F.MUL, which, legal)
        device_run(dc, "dc_bc_", F.IS_ZERO_MOD, which, F.random_rows(F.IS_ZERO_MOD, which, 4096))
        c, _ = read()
        assert not c.any(), c
        a = [10 ** 9] + [0] * 8
        b = [int(F.MUL_LIMB_LIMIT / 10 ** 9) + 2] + [0] * 8
        rows = legal.copy()
        rows[1234] = F.row(a, b)
        device_run(dc, "dc_bc_", F.MUL, which, rows)
        z = F.random_rows(F.IS_ZERO_MOD, which, 4096)
        z[77] = F.row(F.limbs(2 * m))
        device_run(dc, "dc_bc_", F.IS_ZERO_MOD, which, z)
        c, f = read()
        assert c[0] == 1 and c[4] == 1 and c.sum() == 2, c           # KZG_SITE_MUL_LIMBS, KZG_SITE_IS_ZERO_MOD
        assert f[0].tolist() == a and f[4].tolist() == F.limbs(2 * m)


def _tile(rows, n):
    """rows repeated to n, so every case runs at many lane and wave positions of a full-chip launch"""
    return np.ascontiguousarray(np.resize(rows, (n,) + rows.shape[1:]))


@pytest.mark.parametrize("op", range(3), ids=F.CURVE_NAMES)
def test_device_point_formulas_three_ways(dc, hc, op, test_srs_points):  # noqa: F811
    """curve.h on the device (asm and C++ products) == the bound-checked host build, limb for limb, and == the affine group law on
    every case, including the same point, the negated point and the identity (where a violated precondition would pick the wrong
    exceptional branch of xyzz_madd / xyzz_add)."""
    import random
    cases = F.curve_cases(test_srs_points, random.Random(100 + op), 200)
    base = F.curve_rows(cases)
    rows = _tile(base, 1 << 16)
    u32p = C.POINTER(C.c_uint32)
    host = np.zeros((rows.shape[0], 32), np.uint32)
    hc.hc_curve(op, rows.ctypes.data_as(u32p), host.ctypes.data_as(u32p), C.c_size_t(rows.shape[0]))
    for i, (p1, p2, s) in enumerate(cases):
        assert F.xyzz_wire_to_affine(host[i]) == F.curve_expected(op, p1, p2, s), (F.CURVE_NAMES[op], i)
    for prefix in ("dc_cpp_", "dc_asm_"):
        got = np.zeros_like(host)
        rc = getattr(dc, prefix + "curve")(op, rows.ctypes.data_as(u32p), got.ctypes.data_as(u32p), C.c_uint32(rows.shape[0]))
        assert rc == 0, rc
        assert np.array_equal(got, host), (prefix, F.CURVE_NAMES[op], _first_diff(got, host, rows))


def test_device_naf_recoding_matches_the_host(dc, hc):  # noqa: F811
    """naf.h on the device: the digits of every scalar and width equal the host's, and reproduce the scalar (mixed widths and digit
    counts in every wave)."""
    import random
    ks, scal, width = F.naf_rows(random.Random(2024), 600)
    n = 1 << 15
    scal_t, width_t = _tile(scal, n), _tile(width, n)
    u32p = C.POINTER(C.c_uint32)
    host = np.zeros((n, 64), np.uint32)
    hc.hc_naf_rows(scal_t.ctypes.data_as(u32p), width_t.ctypes.data_as(i32p), host.ctypes.data_as(u32p), C.c_size_t(n))
    for i in range(len(width)):
        assert F.naf_value(host[i], int(width[i])) == ks[i // len(F.NAF_WIDTHS)], i
    got = np.zeros_like(host)
    assert dc.dc_asm_naf(scal_t.ctypes.data_as(u32p), width_t.ctypes.data_as(i32p), got.ctypes.data_as(u32p), C.c_uint32(n)) == 0
    assert np.array_equal(got, host), _first_diff(got, host, scal_t)
