"""Per-call time of KZG.compute_multiproofs (FK20, every coset proof in one call) from host buffers, n = 2^12 .. 2^20 at chunk_len 1 and
16, with the SRS cache built first (its build time reported too), next to the per-point loop it replaces: n x KZG.compute_proof_stream
at 2^12 and 2^14, a sample of that loop scaled to n at the larger sizes.  Every timed window ends in a device synchronisation (the
calls return host arrays); each shape is warmed up once.  MP_LOGS / MP_CHUNKS / MP_SAMPLE override the sizes, chunks and sample; MP_OUT names a JSON file for the rows."""
import hashlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
import rust_kzg_bn254_amd as k

ctx = k.Context(0)
logs = [int(x) for x in os.environ.get("MP_LOGS", "12,14,16,18,20").split(",")]
chunks = [int(x) for x in os.environ.get("MP_CHUNKS", "1,16").split(",")]
sample = int(os.environ.get("MP_SAMPLE", "256"))
tau = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % bench.FR
srs = k.SRS.generate(tau, 1 << max(logs), ctx=ctx)
rows = []


def timed(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


for log_n in logs:
    n = 1 << log_n
    poly = k.PolynomialEvalForm(bench.ints_to_wire(bench.uniform_scalars(n, 7)[0]))
    kz = k.KZG.new(ctx)
    kz.calculate_and_store_roots_of_unity(n * 32)
    roots = kz.get_roots_of_unities()
    count = n if log_n <= 14 else min(n, sample)
    list(kz.compute_proof_stream(((poly, roots[i]) for i in range(min(count, 8))), srs))     # warm-up
    t0 = time.perf_counter()
    for _ in kz.compute_proof_stream(((poly, roots[i]) for i in range(count)), srs):
        pass
    per_proof = (time.perf_counter() - t0) / count * 1e3
    loop_ms = per_proof * n
    for l in chunks:
        if l > n // 2:
            continue
        t0 = time.perf_counter()
        srs.cache_multiproof(n, l)
        build_ms = (time.perf_counter() - t0) * 1e3
        kz.compute_multiproofs(poly, srs, l)                                                  # warm-up of this shape
        reps = 5 if log_n <= 16 else 2
        call_ms = timed(lambda: kz.compute_multiproofs(poly, srs, l), reps)
        row = {"n": n, "chunk_len": l, "proofs": n // l, "multiproofs_ms": round(call_ms, 3), "cache_build_ms": round(build_ms, 1),
               "compute_proof_ms_each": round(per_proof, 4), "loop_points": count, "loop_ms_for_n_points": round(loop_ms, 1),
               "speedup_vs_n_point_loop": round(loop_ms / call_ms, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    srs.drop_multiproof()

if os.environ.get("MP_OUT"):                                                                   # all rows as one JSON file
    with open(os.environ["MP_OUT"], "w") as f:
        json.dump(rows, f, indent=1)
