"""Per-call time of KZG.recover_from_cosets (erasure decoding, `kzg_recover_from_cosets`) from host buffers, next to the floor it is made
of: four device-resident Fr NTTs of the same n (`kzg_fr_ntt_device`, two forward and two inverse), measured in the same run.  Shapes:
(n = 2^13, l = 1), (2^16, 64) and (2^20, 16) with every odd coset missing, and (2^20, 16) with one coset missing.  Each shape is a
random polynomial of degree < count * l evaluated with the library's own NTT; the recovered evaluations are compared with it (a round
trip, not an independent check: tests/test_gpu_recover.py has those).  Every timed window ends in a device synchronisation (the call
returns host arrays; the NTT window ends in torch.cuda.synchronize); each shape is warmed up twice; the figure is the median of the
repetitions.  RC_SHAPES="log_n:l:missing,..." (missing = half | one) overrides the shapes, RC_REPS the repetitions, RC_OUT names a JSON file."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import rust_kzg_bn254_amd as k
from rust_kzg_bn254_amd import _lib

lib = _lib.load()
ctx = k.Context(0)
shapes = [s.split(":") for s in os.environ.get("RC_SHAPES", "13:1:half,16:64:half,20:16:half,20:16:one").split(",")]
reps = int(os.environ.get("RC_REPS", "9"))
rows = []


def median_ms(fn, reps, sync=None):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


for log_n, l, missing in shapes:
    n, l = 1 << int(log_n), int(l)
    m = n // l
    ks = np.arange(0, m, 2, dtype=np.uint64) if missing == "half" else np.arange(0, m - 1, dtype=np.uint64)
    count = len(ks)
    rng = np.random.Generator(np.random.PCG64(n + l))
    coeffs = np.zeros((n, 4), dtype=np.uint64)
    coeffs[:count * l] = rng.integers(0, 1 << 60, size=(count * l, 4), dtype=np.uint64)       # < 2^252: canonical wire words
    kz = k.KZG.new(ctx)
    poly = k.PolynomialCoeffForm(coeffs).to_eval_form(ctx)
    ys = np.ascontiguousarray(kz.cosets(poly, l)[ks.astype(np.int64)])
    for _ in range(2):                                                                        # warm-up: tables, workspaces, code objects
        got = kz.recover_from_cosets(ks, ys, n)
    ok = bool(np.array_equal(got.evaluations(), poly.evaluations()))
    call = median_ms(lambda: kz.recover_from_cosets(ks, ys, n), reps)
    call_c = median_ms(lambda: kz.recover_from_cosets(ks, ys, n, eval_form=False), reps)
    d = torch.from_numpy(poly.evaluations().view(np.int64)).to("cuda")
    p = C.c_void_p(d.data_ptr())

    def four_ntts():
        for inv in (1, 0, 1, 0):
            assert lib.kzg_fr_ntt_device(ctx.handle, p, n, inv) == 0

    four_ntts(); torch.cuda.synchronize()
    floor = median_ms(four_ntts, max(reps, 25), torch.cuda.synchronize)
    row = {"n": n, "chunk_len": l, "m": m, "missing": m - count, "vanishing_products": 2 * m * (m - count), "round_trip_ok": ok,
           "recover_eval_form_ms": round(call[0], 3), "min_ms": round(call[1], 3), "max_ms": round(call[2], 3),
           "recover_coeff_form_ms": round(call_c[0], 3), "four_ntts_ms": round(floor[0], 4), "ratio_to_four_ntts": round(call[0] / floor[0], 1),
           "reps": reps}
    rows.append(row)
    print(json.dumps(row), flush=True)
    assert ok, "the recovered evaluations differ from the polynomial's"

if os.environ.get("RC_OUT"):                                                                   # all rows as one JSON file
    with open(os.environ["RC_OUT"], "w") as f:
        json.dump(rows, f, indent=1)
