"""Per-call time of verifier.locate_bad_multiproofs (kzg_verify_multiproof_batch_locate: group sums on the GPU, tree search with one pairing
check per step on the host) against the two things a caller had before it, in the same process on the same box:
  (a) kzg_verify_multiproof_batch on the whole batch (what rejecting costs), and
  (b) one kzg_verify_multiproof_batch call per commitment row with the weights supplied (the only way to name the bad rows before).
Shapes: M commitments x 64 items of chunk_len l on a 4 096-point domain (known-tau SRS), grouped by commitment, with 0, 1 and 8 bad
rows (one value of one item changed per bad row); ML_SHAPES="M,l;M,l" (default "1024,64;64,16").  Weights derived inside the call, items
row-major.  Every timed window is the host clock around a call that ends in a device synchronisation and the host pairings; one warm-up,
median of ML_REPS (7).  The phase split comes from a child process run with KZG_VB_TRACE=1 (the library then synchronises between
phases): median per phase over the calls after the first.  ML_OUT names a JSON file, ML_NO_TRACE=1 skips the child."""
import ctypes as C, hashlib, json, os, re, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
import rust_kzg_bn254_amd as k
from rust_kzg_bn254_amd import _lib, verifier

N_DOMAIN = 4096
PER_ROW = 64
REPS = int(os.environ.get("ML_REPS", "7"))
SHAPES = [tuple(int(v) for v in s.split(",")) for s in os.environ.get("ML_SHAPES", "1024,64;64,16").split(";")]
BAD = (0, 1, 8)
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


def build_items(M, l):
    m = N_DOMAIN // l
    commitments, ys, proofs = [], [], []
    for p in range(M):
        poly = k.PolynomialEvalForm(bench.ints_to_wire(bench.uniform_scalars(N_DOMAIN, 7000 * l + p)[0]))
        commitments.append(kz.commit_eval_form(poly, srs))
        ys.append(kz.cosets(poly, l)[:PER_ROW])
        proofs.append(kz.compute_multiproofs(poly, srs, l)[:PER_ROW])
    assert m >= PER_ROW
    rows = np.repeat(np.arange(M, dtype=np.uint64), PER_ROW)
    ks = np.tile(np.arange(PER_ROW, dtype=np.uint64), M)
    g2 = k.helpers.g2_mul_generator(k.fr.fr_from_int(pow(tau, l, bench.FR)))
    return (np.ascontiguousarray(np.stack(commitments)), rows, ks, np.ascontiguousarray(np.concatenate(ys)), np.ascontiguousarray(np.concatenate(proofs)), g2)


def corrupted(ys, M, bad):
    ys = ys.copy()
    rows = [(r * M) // bad + 3 if bad > 1 else M // 2 for r in range(bad)]
    for r in rows:
        ys[r * PER_ROW + 17, 0] = k.fr.fr_from_int(k.fr.fr_to_int(ys[r * PER_ROW + 17, 0]) + 1)
    return ys, sorted(rows)


def batch_call(cm, ci, ki, ys, pf, g2, l, rp=None, lo=0, hi=None):
    hi = len(ci) if hi is None else hi
    ok = _lib.i32(0)
    rc = _lib.load().kzg_verify_multiproof_batch(ctx.handle, srs.handle, _lib.ptr(cm), len(cm), _lib.ptr(ci[lo:hi]), _lib.ptr(ki[lo:hi]), _lib.ptr(ys[lo:hi]),
                                                 _lib.ptr(pf[lo:hi]), hi - lo, N_DOMAIN, l, None if rp is None else _lib.ptr(rp[lo:hi]), _lib.ptr(g2), C.byref(ok))
    assert rc == 0, rc
    return ok.value


results = []
for M, l in SHAPES:
    cm, ci, ki, ys0, pf, g2 = build_items(M, l)
    N = M * PER_ROW
    for bad in BAD:
        ys, bad_rows = corrupted(ys0, M, bad)
        located = {}

        good = np.zeros(M, np.uint8)
        n_bad, n_checks = _lib.sz(0), _lib.sz(0)

        def locate():                                                                          # (the C entry itself: the Python wrapper's packing of 65 536 items is not the subject)
            rc = _lib.load().kzg_verify_multiproof_batch_locate(ctx.handle, srs.handle, _lib.ptr(cm), M, _lib.ptr(ci), _lib.ptr(ki), _lib.ptr(ys), _lib.ptr(pf), N, N_DOMAIN,
                                                                l, None, _lib.ptr(g2), _lib.ptr(ci), M, good.ctypes.data_as(_lib.u8p), C.byref(n_bad), C.byref(n_checks))
            assert rc == 0, rc
            located["rows"], located["checks"] = [int(r) for r in np.flatnonzero(good == 0)], int(n_checks.value)
        if TRACE_CHILD:
            for _ in range(6):
                locate()
            continue
        locate_ms = median_ms(locate)
        assert located["rows"] == bad_rows, (located, bad_rows)
        whole_ms = median_ms(lambda: batch_call(cm, ci, ki, ys, pf, g2, l))
        rp = verifier.compute_multiproof_r_powers(list(cm), ci, ki, ys, list(pf), N_DOMAIN)

        def per_row():
            found = [r for r in range(M) if not batch_call(cm, ci, ki, ys, pf, g2, l, rp, r * PER_ROW, (r + 1) * PER_ROW)]
            assert found == bad_rows
        per_row_ms = median_ms(per_row, reps=3)
        row = {"commitments": M, "items": N, "chunk_len": l, "values_MiB": round(N * l * 32 / 2**20, 2), "bad_rows": bad, "locate_ms": round(locate_ms, 3),
               "pairing_checks": located["checks"], "batch_call_ms": round(whole_ms, 3), "per_row_loop_ms": round(per_row_ms, 2),
               "locate_over_batch": round(locate_ms / whole_ms, 2), "per_row_loop_over_locate": round(per_row_ms / locate_ms, 1)}
        results.append(row)
        print(json.dumps(row), flush=True)

PHASES = ("plan + r_powers + upload", "interpolation + segment sums", "coefficient MSMs", "point sums", "host sums")
if not TRACE_CHILD and not os.environ.get("ML_NO_TRACE"):
    env = dict(os.environ, KZG_VB_TRACE="1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child"], env=env, capture_output=True, text=True, timeout=1100)
    assert res.returncode == 0, res.stderr[-2000:]
    sums, search = [], []
    for ln in res.stderr.splitlines():
        mt = re.match(r"coset_group_sums N=(\d+) l=(\d+) .*?: (.*)", ln)
        if mt:
            sums.append((int(mt.group(1)), int(mt.group(2)), [float(v) for v in re.findall(r"([0-9.]+) ms", mt.group(3))]))
        mt = re.match(r"kzg_verify_multiproof_batch_locate groups=\d+: search ([0-9.]+) ms", ln)
        if mt:
            search.append(float(mt.group(1)))
    assert len(sums) == len(search) == 6 * len(results), (len(sums), len(search))
    for i, row in enumerate(results):
        calls, srch = sums[6 * i + 1:6 * i + 6], search[6 * i + 1:6 * i + 6]
        assert all(c[0] == row["items"] and c[1] == row["chunk_len"] for c in calls)
        row["traced_phase_ms"] = {name: round(statistics.median(c[2][j] for c in calls), 3) for j, name in enumerate(PHASES)}
        row["traced_phase_ms"]["search"] = round(statistics.median(srch), 3)
        print(json.dumps({"commitments": row["commitments"], "chunk_len": row["chunk_len"], "bad_rows": row["bad_rows"], "traced_phase_ms": row["traced_phase_ms"]}),
              flush=True)

if os.environ.get("ML_OUT") and not TRACE_CHILD:
    with open(os.environ["ML_OUT"], "w") as f:
        json.dump(results, f, indent=1)
