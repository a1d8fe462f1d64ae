"""Per-call time of the G2 MSM (`kzg_msm_g2_srs`, csrc/g2msm.hip) from host buffers at n = 2^12, 2^16 and 2^20 on one MI355X, and beside
each, in the same process, the G1 MSM of the same n in GENERIC mode (an SRS uploaded with KZG_NO_PRECOMPUTE=1: no window or per-bit
tables, the same bucket method with the same window bits).  Also: 4 096 host double-and-add multiplications in G2 (`kzg_validate_g2_point`
runs one `g2_mul` by r each; the sum of 4 096 of them is what a host G2 MSM of 2^12 pairs costs without its additions), and the blob
header call (`kzg_commit_with_length_proof`, two base sets) beside its three parts called one by one, at 2^12 or at every exponent of
G2_HEADER_LG.  Every timed window is a synchronous call that
returns host data; each shape is warmed up twice; the figure is the median of the repetitions (min and max beside it).
G2_SIZES="12,16,20" overrides the sizes, G2_REPS the repetitions, G2_OUT names a JSON file."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["KZG_NO_PRECOMPUTE"] = "1"                    # read at every SRS upload: the G1 handles below carry no tables
import numpy as np
import rust_kzg_bn254_amd as k
from rust_kzg_bn254_amd import _lib, helpers
from rust_kzg_bn254_amd.fr import fr_from_int

lib = _lib.load()
ctx = k.Context(0)
TAU = 0x1D2C3B4A5968778695A4B3C2D1E0F1234567
sizes = [int(s) for s in os.environ.get("G2_SIZES", "12,16,20").split(",")]
reps = int(os.environ.get("G2_REPS", "7"))


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)


out = {"rows": [], "reps": reps}
header_lgs = [int(s) for s in os.environ.get("G2_HEADER_LG", "12").split(",")]
top = 1 << max(sizes + header_lgs)
t0 = time.perf_counter()
g2 = k.G2SRS.generate(TAU, top, ctx=ctx)
out["g2_srs_generate_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
g1 = k.SRS.generate(TAU, top, ctx=ctx)
rng = np.random.Generator(np.random.PCG64(7))
for lg in sizes:
    n = 1 << lg
    sc = np.ascontiguousarray(rng.integers(0, 1 << 60, size=(n, 4), dtype=np.uint64))      # < 2^252: canonical wire words
    o2 = np.zeros(16, np.uint64); o1 = np.zeros(8, np.uint64); inf = C.c_uint8(0)

    def run_g2():
        assert lib.kzg_msm_g2_srs(ctx.handle, g2.handle, 0, _lib.ptr(sc), n, _lib.ptr(o2), C.byref(inf)) == 0

    def run_g1():
        assert lib.kzg_msm_g1_srs(ctx.handle, g1.handle, 0, _lib.ptr(sc), n, _lib.ptr(o1), C.byref(inf)) == 0

    for _ in range(2):
        run_g2(); run_g1()
    # the two results are commitments to the same polynomial
    G1 = k.SRS.generate(TAU, 1, ctx=ctx).g1[0]
    ok = bool(helpers.pairings_verify(o1, helpers.g2_generator(), G1, o2))
    a, b = median_ms(run_g2, reps), median_ms(run_g1, reps)
    out["rows"].append({"n": n, "g2_msm_ms": a[0], "g2_min_ms": a[1], "g2_max_ms": a[2], "g1_generic_msm_ms": b[0], "g1_min_ms": b[1],
                        "g1_max_ms": b[2], "ratio_g2_over_g1": round(a[0] / b[0], 2), "pairing_ok": ok})
    print(out["rows"][-1], flush=True)

# the host's double-and-add in G2: 4 096 multiplications by r (kzg_validate_g2_point: on-curve test, one g2_mul, two comparisons)
pt = helpers.g2_mul_generator(fr_from_int(12345))
reason = C.c_int32(0)
t0 = time.perf_counter()
for _ in range(4096):
    lib.kzg_validate_g2_point(_lib.ptr(pt), C.byref(reason))
out["host_g2_mul_x4096_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
print("host g2_mul x 4096: %.1f ms" % out["host_g2_mul_x4096_ms"], flush=True)

# the header call (nb = 2) beside its three parts, at every length of G2_HEADER_LG
for lg in header_lgs:
    d = 1 << lg
    N = max(1 << 16, d)
    n = d
    trailing = k.G2SRS.generate(TAU, d, first_power=N - d, ctx=ctx)
    sc = np.ascontiguousarray(rng.integers(0, 1 << 60, size=(n, 4), dtype=np.uint64))
    c = np.zeros(8, np.uint64); c2 = np.zeros(16, np.uint64); pi2 = np.zeros(16, np.uint64); inf = C.c_uint8(0)

    def header():
        assert lib.kzg_commit_with_length_proof(ctx.handle, g1.handle, g2.handle, trailing.handle, N - d, N, _lib.ptr(sc), n, d, _lib.ptr(c), _lib.ptr(c2), _lib.ptr(pi2)) == 0

    s1 = np.zeros(8, np.uint64); s2 = np.zeros(16, np.uint64); s3 = np.zeros(16, np.uint64)

    def parts():
        assert lib.kzg_commit_coeff_form(ctx.handle, g1.handle, _lib.ptr(sc), n, _lib.ptr(s1), C.byref(inf)) == 0
        assert lib.kzg_commit_g2_coeff_form(ctx.handle, g2.handle, _lib.ptr(sc), n, _lib.ptr(s2), C.byref(inf)) == 0
        assert lib.kzg_msm_g2_srs(ctx.handle, trailing.handle, 0, _lib.ptr(sc), n, _lib.ptr(s3), C.byref(inf)) == 0

    for _ in range(2):
        header(); parts()
    assert np.array_equal(c, s1) and np.array_equal(c2, s2) and np.array_equal(pi2, s3)
    h, p = median_ms(header, reps), median_ms(parts, reps)
    out["header_2_%d" % lg] = {"n": n, "header_call_ms": h[0], "min_ms": h[1], "max_ms": h[2], "three_parts_ms": p[0], "parts_min_ms": p[1], "parts_max_ms": p[2]}
    print(out["header_2_%d" % lg], flush=True)
if os.environ.get("G2_OUT"):
    os.makedirs(os.path.dirname(os.path.abspath(os.environ["G2_OUT"])), exist_ok=True)
    json.dump(out, open(os.environ["G2_OUT"], "w"), indent=1)
