"""Per-call time of verifier.verify_multiproof_batch (coset proofs of KZG.compute_multiproofs, one pairing check per batch) on a known-tau
SRS: rows N in {256, 4096, 65536} x chunk_len in {1, 16, 64}, with the weights derived inside the call and, separately, supplied.
Items are distinct proofs of ceil(N / m) random polynomials of n = 2^16 evaluations (m = n / chunk_len cosets each).  Every timed
window is the host clock around a call that ends in a device synchronisation and the host pairing; one warm-up, median of MV_REPS (7).

The phase split (r_powers / upload / interpolation kernel / coefficient MSM / proof and commitment MSMs / point sums and pairing)
comes from a child process run with KZG_VB_TRACE=1 (the library then synchronises between phases, so those calls are slower than the
timed ones): median per phase.  The gate row (chunk_len 1, N 4096) is compared with 4096 calls of kzg_verify_proof and with
kzg_verify_kzg_proof_batch of the same items, both taken from the library named by MV_BASELINE_LIB (the build of the parent commit;
default: this build, whose code for the two is the same).
MV_ROWS="N,l;N,l" restricts the rows (e.g. for a profiler run), MV_OUT names a JSON file, MV_NO_TRACE=1 skips the child."""
import ctypes as C, hashlib, json, os, re, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
import rust_kzg_bn254_amd as k
from rust_kzg_bn254_amd import _lib, verifier

LOG_N = 16
N_DOMAIN = 1 << LOG_N
REPS = int(os.environ.get("MV_REPS", "7"))
ROWS = [(N, l) for l in (1, 16, 64) for N in (256, 4096, 65536)]
if os.environ.get("MV_ROWS"):
    ROWS = [tuple(int(v) for v in r.split(",")) for r in os.environ["MV_ROWS"].split(";")]
TRACE_CHILD = "--trace-child" in sys.argv
tau = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % bench.FR
ctx = k.Context(0)
srs = k.SRS.generate(tau, N_DOMAIN, ctx=ctx)
kz = k.KZG.new(ctx)
kz.calculate_and_store_roots_of_unity(N_DOMAIN * 32)


def median_ms(fn, reps=REPS):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def build_items(N, l):
    m = N_DOMAIN // l
    polys = -(-N // m)
    commitments, ys, proofs, rows, ks = [], [], [], [], []
    for p in range(polys):
        poly = k.PolynomialEvalForm(bench.ints_to_wire(bench.uniform_scalars(N_DOMAIN, 100 * l + p)[0]))
        take = min(m, N - p * m)
        commitments.append(kz.commit_eval_form(poly, srs))
        ys.append(kz.cosets(poly, l)[:take])
        proofs.append(kz.compute_multiproofs(poly, srs, l)[:take])
        rows += [p] * take
        ks += list(range(take))
    g2 = k.helpers.g2_mul_generator(k.fr.fr_from_int(pow(tau, l, bench.FR)))
    return (np.ascontiguousarray(np.stack(commitments)), np.array(rows, np.uint64), np.array(ks, np.uint64), np.ascontiguousarray(np.concatenate(ys)),
            np.ascontiguousarray(np.concatenate(proofs)), g2)


def batch_call(items, N, l, rp):
    cm, ci, ki, ys, pf, g2 = items
    ok = _lib.i32(0)
    rc = _lib.load().kzg_verify_multiproof_batch(ctx.handle, srs.handle, _lib.ptr(cm), len(cm), _lib.ptr(ci), _lib.ptr(ki), _lib.ptr(ys), _lib.ptr(pf), N,
                                                 N_DOMAIN, l, None if rp is None else _lib.ptr(rp), _lib.ptr(g2), C.byref(ok))
    assert rc == 0 and ok.value == 1, (rc, ok.value)


def baseline(items, N):
    """4096 x kzg_verify_proof and one kzg_verify_kzg_proof_batch over the same (C, w^k, y, proof) rows with the baseline library."""
    path = os.environ.get("MV_BASELINE_LIB") or _lib.LIB_PATH
    lib = C.CDLL(path)
    u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    lib.kzg_verify_proof.argtypes = [u64p] * 5 + [i32p]
    lib.kzg_verify_kzg_proof_batch.argtypes = [C.c_void_p] + [u64p] * 5 + [C.c_size_t, u64p, i32p]
    lib.kzg_compute_r_powers.argtypes = [u64p] * 5 + [C.c_size_t, u64p]
    lib.kzg_ctx_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
    lib.kzg_ctx_destroy.argtypes = [C.c_void_p]
    cm, ci, ki, ys, pf, g2 = items
    roots = np.ascontiguousarray(kz.get_roots_of_unities())
    cs = np.ascontiguousarray(cm[ci.astype(np.int64)])
    zs = np.ascontiguousarray(roots[ki.astype(np.int64)])
    y1 = np.ascontiguousarray(ys.reshape(N, 4))
    ok = C.c_int32(0)
    P = lambda a: a.ctypes.data_as(u64p)                                                       # noqa: E731

    def loop():
        for i in range(N):
            rc = lib.kzg_verify_proof(P(cs[i]), P(pf[i]), P(y1[i]), P(zs[i]), P(g2), C.byref(ok))
            assert rc == 0 and ok.value == 1
    t0 = time.perf_counter()
    loop()
    loop_ms = (time.perf_counter() - t0) * 1e3
    h = C.c_void_p()
    assert lib.kzg_ctx_create(0, C.byref(h)) == 0
    lens = np.full(N, N_DOMAIN, np.uint64)
    rp = np.zeros((N, 4), np.uint64)

    def batch():
        assert lib.kzg_compute_r_powers(P(cs), P(zs), P(y1), P(pf), P(lens), N, P(rp)) == 0
        assert lib.kzg_verify_kzg_proof_batch(h, P(cs), P(zs), P(y1), P(pf), P(rp), N, P(g2), C.byref(ok)) == 0 and ok.value == 1
    batch_ms = median_ms(batch)
    lib.kzg_ctx_destroy(h)
    return {"baseline_lib": os.path.relpath(path, ROOT), "verify_proof_loop_ms": round(loop_ms, 1), "verify_proof_ms_each": round(loop_ms / N, 4),
            "verify_kzg_proof_batch_ms": round(batch_ms, 3)}


PHASES = ("r_powers", "upload", "interpolation kernel", "coefficient MSM", "host scalars + proof / commitment MSMs", "point sums + pairing", "call")
results = []
for N, l in ROWS:
    items = build_items(N, l)
    if TRACE_CHILD:
        for _ in range(6):                                                                     # the first is the warm-up the parent drops
            batch_call(items, N, l, None)
        continue
    derived_ms = median_ms(lambda: batch_call(items, N, l, None))
    rp = verifier.compute_multiproof_r_powers(list(items[0]), items[1], items[2], items[3], list(items[4]), N_DOMAIN)
    supplied_ms = median_ms(lambda: batch_call(items, N, l, rp))
    row = {"N": N, "chunk_len": l, "n": N_DOMAIN, "commitments": len(items[0]), "values_MiB": round(N * l * 32 / 2**20, 2),
           "batch_ms_r_derived": round(derived_ms, 3), "batch_ms_r_supplied": round(supplied_ms, 3)}
    if (N, l) == (4096, 1):
        row.update(baseline(items, N))
        row["speedup_vs_verify_proof_loop"] = round(row["verify_proof_loop_ms"] / derived_ms, 1)
        row["ratio_to_verify_kzg_proof_batch"] = round(derived_ms / row["verify_kzg_proof_batch_ms"], 2)
    results.append(row)
    print(json.dumps(row), flush=True)

if not TRACE_CHILD and not os.environ.get("MV_NO_TRACE"):
    env = dict(os.environ, KZG_VB_TRACE="1", MV_ROWS=";".join("%d,%d" % r for r in ROWS))
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child"], env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    seen = {}
    for ln in res.stderr.splitlines():
        mt = re.match(r"kzg_verify_multiproof_batch N=(\d+) l=(\d+) M=\d+: (.*)", ln)
        if mt:
            vals = [float(v) for v in re.findall(r"([0-9.]+) ms", mt.group(3))]
            seen.setdefault((int(mt.group(1)), int(mt.group(2))), []).append(vals)
    for row in results:
        calls = seen.get((row["N"], row["chunk_len"]), [])[1:]
        if calls:
            row["traced_phase_ms"] = {name: round(statistics.median(c[i] for c in calls), 3) for i, name in enumerate(PHASES)}
            ker = row["traced_phase_ms"]["interpolation kernel"]
            row["interpolation_GB_per_s"] = round(row["N"] * row["chunk_len"] * 32 / 1e9 / (ker / 1e3), 1) if ker > 0 else None
            row["interpolation_share_of_traced_call"] = round(ker / row["traced_phase_ms"]["call"], 3)
            print(json.dumps({"N": row["N"], "chunk_len": row["chunk_len"], "traced_phase_ms": row["traced_phase_ms"],
                              "interpolation_GB_per_s": row["interpolation_GB_per_s"]}), flush=True)

if os.environ.get("MV_OUT") and not TRACE_CHILD:
    with open(os.environ["MV_OUT"], "w") as f:
        json.dump(results, f, indent=1)
