"""Per-call time of KZG.prove_cosets (the values and proofs of k selected cosets of one blob: one division and one commitment per coset)
next to KZG.encode_cosets (every coset, FK20) in the same process on the same SRS, at the shapes of profiles/encode.md: d = 2^12 r = 8
l = 16; d = 2^14 r = 8 l in {1, 16}; d = 2^16 r = 8 l in {1, 16}; k in {1, 2, 4, 16, 64, 256}.  Per (shape, k): the whole call, the call
with proofs only, the call with values only (the field passes without the quotient rows, the l-point transforms, the download), and the
MSM alone on the same quotient rows resident on the device (kzg_commit_coeff_form_batch_device: the batched path of the call) -- the
field passes and the MSM as separate figures.  For k = 1 the quotient row also goes through kzg_msm_g1_srs_device (the single MSM), the
two paths alternating call by call.  The FK20 table and the SRS's per-bit tables are built before anything is timed; one warm-up per
timed call, PC_REPS repetitions (default 9), host clock around calls that end in a device synchronisation; median, min and max are
recorded.  PC_SHAPES ("log_d:r:l,...") / PC_KS / PC_REPS override; PC_OUT names a JSON file for the rows.  Needs torch for the resident
rows."""
import ctypes as C, hashlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch                                                                                   # before the library (load order: tests/conftest.py)
import bench
import rust_kzg_bn254_amd as k

L = k._lib
lib = L.load()
ctx = k.Context(0)
shapes = [tuple(int(v) for v in s.split(":")) for s in os.environ.get("PC_SHAPES", "12:8:16,14:8:1,14:8:16,16:8:1,16:8:16").split(",")]
ks = [int(x) for x in os.environ.get("PC_KS", "1,2,4,16,64,256").split(",")]
reps = int(os.environ.get("PC_REPS", "9"))
tau = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % bench.FR
rows = []


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(times):
    return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4)}


def measure(fn):
    fn()                                                                                       # warm-up of this call
    return stats([timed(fn) for _ in range(reps)])


def measure_alternating(fa, fb):
    fa(); fb()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fa))
        tb.append(timed(fb))
    return stats(ta), stats(tb)


kz = k.KZG.new(ctx)
for log_d in sorted({s[0] for s in shapes}):
    d = 1 << log_d
    srs = k.SRS.generate(tau, d, ctx=ctx)                                                      # the prover and the encoder need d points
    coeffs = bench.ints_to_wire(bench.uniform_scalars(d, 7)[0])
    poly = k.PolynomialCoeffForm(coeffs)
    for (ld, r, l) in shapes:
        if ld != log_d:
            continue
        n, m = d * r, d * r // l
        srs.cache_multiproof(d, l)
        enc = measure(lambda: kz.encode_cosets(poly, srs, n, l))
        rnd = np.random.default_rng(1000 * log_d + l)
        for kk in ks:
            if kk > m:
                continue
            items = [int(x) for x in rnd.choice(m, size=kk, replace=False)]
            both = measure(lambda: kz.prove_cosets(poly, srs, n, items, l))
            proofs_only = measure(lambda: kz.prove_cosets(poly, srs, n, items, l, values=False))
            values_only = measure(lambda: kz.prove_cosets(poly, srs, n, items, l, proofs=False))
            # the MSM alone: the same quotient rows, resident
            q, _ = kz.coset_quotients(poly, n, None, items, l)
            want = kz.prove_cosets(poly, srs, n, items, l, values=False)[1]
            dq = torch.from_numpy(q.view(np.int64)).to("cuda:0")
            torch.cuda.synchronize()
            out = np.zeros((kk, 8), dtype=np.uint64)
            inf = np.zeros(kk, dtype=np.uint8)

            def msm_batched():
                rc = lib.kzg_commit_coeff_form_batch_device(ctx.handle, srs.handle, dq.data_ptr(), d, kk, L.ptr(out), inf.ctypes.data_as(L.u8p))
                assert rc == 0, rc

            msm = measure(msm_batched)
            assert np.array_equal(out, want)                                                   # the figures belong to the same bits
            row = {"d": d, "r": r, "n": n, "chunk_len": l, "cosets": m, "k": kk, "encode_all": enc, "prove": both, "prove_proofs_only": proofs_only,
                   "prove_values_only": values_only, "msm_alone_batched": msm,
                   "proofs_only_minus_msm_ms": round(proofs_only["median_ms"] - msm["median_ms"], 4),
                   "encode_over_prove": round(enc["median_ms"] / both["median_ms"], 2), "items_per_group": k.helpers.prove_cosets_info(d, n, l, kk)["items_per_group"]}
            if kk == 1:
                one = np.zeros(8, dtype=np.uint64)
                one_inf = C.c_uint8(0)

                def msm_single():
                    rc = lib.kzg_msm_g1_srs_device(ctx.handle, srs.handle, 0, dq.data_ptr(), d, L.ptr(one), C.byref(one_inf))
                    assert rc == 0, rc

                single, batched = measure_alternating(msm_single, msm_batched)
                assert np.array_equal(one, want[0])
                row["k1_msm_single"] = single
                row["k1_msm_batched"] = batched
                row["k1_planner_takes_single"] = k.helpers.prove_cosets_info(d, n, l, 1)["msm_single"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            del dq
        srs.drop_multiproof()
    srs.close()

# the crossover per shape: the largest measured k at which the direct route is still faster than encoding everything
for (ld, r, l) in shapes:
    mine = [x for x in rows if x["d"] == 1 << ld and x["r"] == r and x["chunk_len"] == l]
    wins = [x["k"] for x in mine if x["prove"]["median_ms"] < x["encode_all"]["median_ms"]]
    loses = [x["k"] for x in mine if x["prove"]["median_ms"] >= x["encode_all"]["median_ms"]]
    print(json.dumps({"d": 1 << ld, "r": r, "chunk_len": l, "direct_wins_up_to_k": max(wins) if wins else None, "direct_loses_from_k": min(loses) if loses else None}), flush=True)

if os.environ.get("PC_OUT"):                                                                   # all rows as one JSON file
    with open(os.environ["PC_OUT"], "w") as f:
        json.dump(rows, f, indent=1)
