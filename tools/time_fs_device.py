"""Per-call time of kzg_verify_multiproof_batch with the weights derived inside the call, the item digests of the transcript hashed on the
host pool against on the device (csrc/fsdevice.hip), beside the same call of the PARENT commit's library in the same process:
rows N in {256, 4096, 65536} x chunk_len in {1, 16, 64}, items as tools/time_multiproof_verify.py builds them (n = 2^16, known-tau SRS).

Four variants per row, taken in turns inside one loop so that drift of the machine hits them alike: `parent` (the library named by
MV_BASELINE_LIB, its own context and SRS), and this build with kzg_ctx_set_transcript_device = 1 (`host`), 2 (`device`), 0 (`auto`).  One
warm-up each, then MV_REPS (7) rounds; median, minimum and maximum per variant (the spread), host clock around a call that ends in a device
synchronisation and the host pairing.  The phase split comes from a child process with KZG_VB_TRACE=1 (the library then synchronises
between phases): median per phase of five calls per variant.

The gate of the rows (65536, 64) and (65536, 16): device <= parent - parent's traced r_powers / 2.  Automatic mode's envelope
(coset_transcript_on_device of csrc/host_fiat_shamir.h) is the set of measured rows where device beats host; rows of few long items
(MV_ROWS="256,256;64,1024") show what it keeps out.  MV_ROWS="N,l;N,l" restricts the rows, MV_OUT names a JSON file, MV_NO_TRACE=1 skips the child, FS_VARIANTS="device" restricts the
variants (a profiler run of one kernel)."""
import ctypes as C, hashlib, json, os, re, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
import rust_kzg_bn254_amd as k
from rust_kzg_bn254_amd import _lib

LOG_N = 16
N_DOMAIN = 1 << LOG_N
REPS = int(os.environ.get("MV_REPS", "7"))
ROWS = [(N, l) for l in (1, 16, 64) for N in (256, 4096, 65536)]
if os.environ.get("MV_ROWS"):
    ROWS = [tuple(int(v) for v in r.split(",")) for r in os.environ["MV_ROWS"].split(";")]
VARIANTS = [v for v in ("parent", "host", "device", "auto") if v in os.environ.get("FS_VARIANTS", "parent,host,device,auto").split(",")]
MODE = {"host": 1, "device": 2, "auto": 0}
TRACE_CHILD = "--trace-child" in sys.argv
tau = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % bench.FR
ctx = k.Context(0)
srs = k.SRS.generate(tau, N_DOMAIN, ctx=ctx)
kz = k.KZG.new(ctx)
kz.calculate_and_store_roots_of_unity(N_DOMAIN * 32)
u64p, vp = C.POINTER(C.c_uint64), C.c_void_p
BATCH_ARGS = [vp, vp, u64p, C.c_size_t, u64p, u64p, u64p, u64p, C.c_size_t, C.c_size_t, C.c_size_t, u64p, u64p, C.POINTER(C.c_int32)]

parent = None
if "parent" in VARIANTS:
    path = os.environ.get("MV_BASELINE_LIB")
    assert path and os.path.exists(path), "MV_BASELINE_LIB must name the parent commit's library"
    plib = C.CDLL(path)
    plib.kzg_ctx_create.argtypes = [C.c_int32, C.POINTER(vp)]
    plib.kzg_srs_generate.argtypes = [vp, u64p, C.c_uint64, C.c_size_t, C.POINTER(vp)]
    plib.kzg_verify_multiproof_batch.argtypes = BATCH_ARGS
    pctx, psrs = vp(), vp()
    assert plib.kzg_ctx_create(0, C.byref(pctx)) == 0
    assert plib.kzg_srs_generate(pctx, _lib.ptr(k.fr.fr_from_int(tau)), 0, N_DOMAIN, C.byref(psrs)) == 0
    parent = (plib, pctx, psrs, os.path.relpath(path, ROOT))


def build_items(N, l):
    m = N_DOMAIN // l
    commitments, ys, proofs, rows, ks = [], [], [], [], []
    for p in range(-(-N // m)):
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


def call(variant, items, N, l):
    cm, ci, ki, ys, pf, g2 = items
    ok = C.c_int32(0)
    P = _lib.ptr
    if variant == "parent":
        lib, h, s = parent[0], parent[1], parent[2]
    else:
        ctx.set_transcript_device(MODE[variant])
        lib, h, s = _lib.load(), ctx.handle, srs.handle
    rc = lib.kzg_verify_multiproof_batch(h, s, P(cm), len(cm), P(ci), P(ki), P(ys), P(pf), N, N_DOMAIN, l, None, P(g2), C.byref(ok))
    assert rc == 0 and ok.value == 1, (variant, rc, ok.value)


PHASES = ("r_powers", "upload", "interpolation kernel", "coefficient MSM", "host scalars + proof / commitment MSMs", "point sums + pairing", "call")
results = []
for N, l in ROWS:
    items = build_items(N, l)
    if TRACE_CHILD:
        for v in VARIANTS:
            print("VARIANT %s" % v, file=sys.stderr, flush=True)
            for _ in range(6):                                                                     # the first is the warm-up the parent process drops
                call(v, items, N, l)
        continue
    for v in VARIANTS:
        call(v, items, N, l)
    times = {v: [] for v in VARIANTS}
    for _ in range(REPS):
        for v in VARIANTS:
            t0 = time.perf_counter()
            call(v, items, N, l)
            times[v].append((time.perf_counter() - t0) * 1e3)
    row = {"N": N, "chunk_len": l, "n": N_DOMAIN, "commitments": len(items[0]), "values_bytes": N * l * 32}
    for v in VARIANTS:
        row[v + "_ms"] = {"median": round(statistics.median(times[v]), 3), "min": round(min(times[v]), 3), "max": round(max(times[v]), 3)}
    results.append(row)
    print(json.dumps(row), flush=True)
ctx.set_transcript_device(0)

if not TRACE_CHILD and not os.environ.get("MV_NO_TRACE"):
    env = dict(os.environ, KZG_VB_TRACE="1", MV_ROWS=";".join("%d,%d" % r for r in ROWS))
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child"], env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    seen, variant = {}, None
    for ln in res.stderr.splitlines():
        if ln.startswith("VARIANT "):
            variant = ln.split()[1]
        mt = re.match(r"kzg_verify_multiproof_batch N=(\d+) l=(\d+) M=\d+: (.*)", ln)
        if mt:
            vals = [float(x) for x in re.findall(r"([0-9.]+) ms", mt.group(3))]
            path = re.match(r"r_powers( \([^)]*\))?", mt.group(3)).group(1)
            seen.setdefault((int(mt.group(1)), int(mt.group(2)), variant), []).append((vals, (path or "").strip()))
    for row in results:
        for v in VARIANTS:
            calls = seen.get((row["N"], row["chunk_len"], v), [])[1:]
            if calls:
                row[v + "_traced_phase_ms"] = {name: round(statistics.median(c[0][i] for c in calls), 3) for i, name in enumerate(PHASES)}
                row[v + "_r_powers_path"] = calls[-1][1]
        if (row["N"], row["chunk_len"]) in ((65536, 64), (65536, 16)) and "parent" in VARIANTS and "device" in VARIANTS and row.get("parent_traced_phase_ms"):
            bound = row["parent_ms"]["median"] - row["parent_traced_phase_ms"]["r_powers"] / 2
            row["gate_bound_ms"] = round(bound, 3)
            row["gate_met"] = row["device_ms"]["median"] <= bound
        print(json.dumps({kk: vv for kk, vv in row.items() if "traced" in kk or "gate" in kk or "path" in kk or kk in ("N", "chunk_len")}), flush=True)

if os.environ.get("MV_OUT") and not TRACE_CHILD:
    with open(os.environ["MV_OUT"], "w") as f:
        json.dump(results, f, indent=1)
