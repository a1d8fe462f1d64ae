"""Per-call time of KZG.encode_cosets (the cosets of values and their proofs for d coefficients on n = r d points) next to the call it
replaces, KZG.compute_multiproofs of the coefficients zero-padded to n, in the same process on the same SRS of n points: d = 2^12, 2^14,
2^16, r = 1, 2, 8, chunk_len 1 and 16.  Per shape the FK20 table of each call is built first (the (d, l) entry for the encoder, the
(n, l) entry for the padded call; build times reported), each call is warmed up once, then timed 5 times; the median is reported.
Every timed window ends in a device synchronisation (the calls return host arrays).  The padded call returns no values: the encoder is
also timed with proofs only.  ENC_LOGS / ENC_RATES / ENC_CHUNKS / ENC_REPS override the shapes and repetitions; ENC_OUT names a JSON
file for the rows."""
import hashlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
import rust_kzg_bn254_amd as k

ctx = k.Context(0)
logs = [int(x) for x in os.environ.get("ENC_LOGS", "12,14,16").split(",")]
rates = [int(x) for x in os.environ.get("ENC_RATES", "1,2,8").split(",")]
chunks = [int(x) for x in os.environ.get("ENC_CHUNKS", "1,16").split(",")]
reps = int(os.environ.get("ENC_REPS", "5"))
tau = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % bench.FR
rows = []


def median_ms(fn):
    fn()                                                                                       # warm-up of this shape
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def build_ms(srs, n, l):
    srs.drop_multiproof()
    t0 = time.perf_counter()
    srs.cache_multiproof(n, l)
    return (time.perf_counter() - t0) * 1e3


kz = k.KZG.new(ctx)
for n in sorted({(1 << log_d) * r for log_d in logs for r in rates}):
    srs = k.SRS.generate(tau, n, ctx=ctx)
    for log_d in logs:
        d = 1 << log_d
        if n % d or n // d not in rates:
            continue
        r = n // d
        coeffs = bench.ints_to_wire(bench.uniform_scalars(d, 7)[0])
        poly = k.PolynomialCoeffForm(coeffs)
        padded = k.PolynomialCoeffForm(np.concatenate([coeffs, np.zeros((n - d, 4), dtype=np.uint64)]))
        for l in chunks:
            enc_build = build_ms(srs, d, l)
            enc = median_ms(lambda: kz.encode_cosets(poly, srs, n, l))
            enc_proofs = median_ms(lambda: kz.encode_cosets(poly, srs, n, l, values=False))
            pad_build = build_ms(srs, n, l)
            pad = median_ms(lambda: kz.compute_multiproofs(padded, srs, l))
            srs.drop_multiproof()
            row = {"d": d, "r": r, "n": n, "chunk_len": l, "cosets": n // l, "encode_ms": round(enc, 3), "encode_proofs_only_ms": round(enc_proofs, 3),
                   "encode_cache_build_ms": round(enc_build, 1), "padded_multiproofs_ms": round(pad, 3), "padded_cache_build_ms": round(pad_build, 1),
                   "padded_over_encode": round(pad / enc, 2), "padded_over_encode_proofs_only": round(pad / enc_proofs, 2)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    srs.close()

if os.environ.get("ENC_OUT"):                                                                  # all rows as one JSON file
    with open(os.environ["ENC_OUT"], "w") as f:
        json.dump(sorted(rows, key=lambda x: (x["d"], x["r"], x["chunk_len"])), f, indent=1)
