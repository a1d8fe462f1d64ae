"""Per-blob time of the batched encoder (kzg_encode_cosets_batch) next to the loop of B kzg_encode_cosets calls over the same blobs, in
one process on one SRS of d points, with the FK20 table built and both calls warmed up: d = 2^12, 2^14, 2^16, r = 1, 2, 8, chunk_len 1
and 16, B = 1, 4, 16, 64.  Both sides go through the C-ABI with preallocated outputs (no allocation inside a timed window); every
timed window ends in a device synchronisation (the calls return host arrays).  Per row: the median of ENCB_REPS (5) repetitions and
their spread (min - max) of each side, the per-blob time, the ratio loop / batch, and the plan kzg_encode_cosets_batch_info reports.
Rows whose output arrays exceed ENCB_MAX_OUT_BYTES (2 GiB) are left out and listed.  ENCB_LOGS / ENCB_RATES / ENCB_CHUNKS / ENCB_COUNTS
override the shapes; ENCB_OUT names a JSON file for the rows.

ENCB_BASELINE_LIB=<the parent commit's library>: instead, the single call (kzg_encode_cosets) at the chunk_len = 16 rows through that
library (its own context and SRS) and through this one, taken in turns in this process, ENCB_REPS repetitions per turn, two turns each:
median and spread of each side.

--render FILE.json [SINGLE.json]: the markdown tables of profiles/encode_batch.md from recorded rows (the ENCB_OUT files of the two
modes, or profiles/encode_batch.json, which holds both); no GPU."""
import hashlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def plan_text(t):
    if t["form"] == "none":
        return "-"
    return "%s on %s, %d stages, %s" % (t["form"], "pairs" if t["pairs"] else "lanes", t["stages"], t["load"])


def render(argv):
    rows = json.load(open(argv[0]))
    singles = json.load(open(argv[1])) if len(argv) > 1 else []
    if isinstance(rows, dict):                                                                 # profiles/encode_batch.json: both tables in one file
        rows, singles = rows["rows"], rows.get("single_call_against_parent", singles)
    log = lambda v: "2^%d" % (v.bit_length() - 1)
    print("| d | r | chunk l | B | groups x blobs | batch, per call | spread | loop, per call | spread | batch per blob | loop per blob | loop / batch | inverse G1 FFT | forward G1 FFT |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %d | %d | %d x %d%s | %.2f ms | %.2f - %.2f | %.2f ms | %.2f - %.2f | %.3f ms | %.3f ms | %.2fx | %s | %s |" % (
            log(r["d"]), r["r"], r["chunk_len"], r["count"], r["groups"], r["blobs_per_group"], "" if r["batched"] else " (rule)", r["batch_ms"],
            r["batch_min_ms"], r["batch_max_ms"], r["loop_ms"], r["loop_min_ms"], r["loop_max_ms"], r["batch_ms"] / r["count"],
            r["loop_ms"] / r["count"], r["loop_over_batch"], plan_text(r["inverse"]), plan_text(r["forward"])))
    if singles:
        print()
        print("| d | r | chunk l | parent: median | min - max | this commit: median | min - max |")
        print("|---|---|---|---|---|---|---|")
        for r in singles:
            print("| %s | %d | %d | %.3f ms | %.3f - %.3f | %.3f ms | %.3f - %.3f |" % (log(r["d"]), r["r"], r["chunk_len"], r["parent_ms"], r["parent_min_ms"],
                                                                             r["parent_max_ms"], r["this_ms"], r["this_min_ms"], r["this_max_ms"]))


if len(sys.argv) > 2 and sys.argv[1] == "--render":
    render(sys.argv[2:])
    sys.exit(0)

import numpy as np
import bench
import rust_kzg_bn254_amd as k

L = k._lib
lib = L.load()
ctx = k.Context(0)
logs = [int(x) for x in os.environ.get("ENCB_LOGS", "12,14,16").split(",")]
rates = [int(x) for x in os.environ.get("ENCB_RATES", "1,2,8").split(",")]
single_only = bool(os.environ.get("ENCB_BASELINE_LIB"))
chunks = [int(x) for x in os.environ.get("ENCB_CHUNKS", "16" if single_only else "1,16").split(",")]
counts = [int(x) for x in os.environ.get("ENCB_COUNTS", "1,4,16,64").split(",")]
reps = int(os.environ.get("ENCB_REPS", "5"))
max_out = int(os.environ.get("ENCB_MAX_OUT_BYTES", str(2 << 30)))
tau = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % bench.FR
rows, skipped = [], []


def times_of(fn):
    fn()                                                                                       # warm-up of this shape
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def timed(fn):
    times = times_of(fn)
    return statistics.median(times), min(times), max(times)


parent = None
if single_only:                                                                                # the parent's library: raw ctypes, its own context
    import ctypes as C
    plib = C.CDLL(os.environ["ENCB_BASELINE_LIB"])
    plib.kzg_ctx_create.argtypes = [C.c_int32, C.POINTER(L.vp)]
    plib.kzg_srs_generate.argtypes = [L.vp, L.u64p, C.c_uint64, C.c_size_t, C.POINTER(L.vp)]
    plib.kzg_srs_cache_multiproof.argtypes = [L.vp, L.vp, L.sz, L.sz]
    plib.kzg_srs_drop_multiproof.argtypes = [L.vp, L.vp]
    plib.kzg_encode_cosets.argtypes = L.PROTOTYPES["kzg_encode_cosets"][1]
    plib.kzg_srs_free.argtypes = [L.vp]
    plib.kzg_srs_free.restype = None
    pctx = L.vp()
    assert plib.kzg_ctx_create(0, C.byref(pctx)) == 0


for log_d in logs:
    d = 1 << log_d
    srs = k.SRS.generate(tau, d, ctx=ctx)
    if single_only:
        psrs = L.vp()
        assert plib.kzg_srs_generate(pctx, L.ptr(k.fr.fr_from_int(tau)), 0, d, C.byref(psrs)) == 0
    bmax = max(counts)
    blobs = np.ascontiguousarray(np.stack([bench.ints_to_wire(bench.uniform_scalars(d, 7 + b)[0]) for b in range(1 if single_only else bmax)]), dtype=np.uint64)
    for r in rates:
        n = d * r
        for l in chunks:
            m = n // l
            srs.cache_multiproof(d, l)
            for B in ([1] if single_only else counts):
                if B * (n * 32 + m * 65) > max_out:
                    skipped.append({"d": d, "r": r, "chunk_len": l, "count": B})
                    continue
                ys = np.zeros((B, m, l, 4), dtype=np.uint64)
                out = np.zeros((B, m, 8), dtype=np.uint64)
                inf = np.zeros((B, m), dtype=np.uint8)

                def loop():
                    for b in range(B):
                        rc = lib.kzg_encode_cosets(ctx.handle, srs.handle, L.ptr(blobs[b]), d, 0, n, l, L.ptr(ys[b]), L.ptr(out[b]), inf[b].ctypes.data_as(L.u8p))
                        assert rc == 0, rc

                if single_only:
                    assert plib.kzg_srs_cache_multiproof(pctx, psrs, d, l) == 0

                    def parent_call():
                        rc = plib.kzg_encode_cosets(pctx, psrs, L.ptr(blobs[0]), d, 0, n, l, L.ptr(ys[0]), L.ptr(out[0]), inf[0].ctypes.data_as(L.u8p))
                        assert rc == 0, rc

                    tp, tt = [], []
                    for _ in range(2):                                                         # taken in turns
                        tp += times_of(parent_call)
                        tt += times_of(loop)
                    assert plib.kzg_srs_drop_multiproof(pctx, psrs) == 0
                    row = {"d": d, "r": r, "n": n, "chunk_len": l, "parent_ms": round(statistics.median(tp), 3), "parent_min_ms": round(min(tp), 3),
                           "parent_max_ms": round(max(tp), 3), "this_ms": round(statistics.median(tt), 3), "this_min_ms": round(min(tt), 3), "this_max_ms": round(max(tt), 3)}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    continue
                lo = timed(loop)
                want = (ys.copy(), out.copy(), inf.copy())

                def batch():
                    rc = lib.kzg_encode_cosets_batch(ctx.handle, srs.handle, L.ptr(blobs), B, d, 0, n, l, L.ptr(ys), L.ptr(out), inf.ctypes.data_as(L.u8p))
                    assert rc == 0, rc

                ba = timed(batch)
                assert np.array_equal(ys, want[0]) and np.array_equal(out, want[1]) and np.array_equal(inf, want[2]), "batch differs from the loop"
                info = k.helpers.encode_batch_info(d, n, l, B)
                row = {"d": d, "r": r, "n": n, "chunk_len": l, "count": B, "batch_ms": round(ba[0], 3), "batch_min_ms": round(ba[1], 3), "batch_max_ms": round(ba[2], 3),
                       "loop_ms": round(lo[0], 3), "loop_min_ms": round(lo[1], 3), "loop_max_ms": round(lo[2], 3), "batch_per_blob_ms": round(ba[0] / B, 4),
                       "loop_per_blob_ms": round(lo[0] / B, 4), "loop_over_batch": round(lo[0] / ba[0], 3), "blobs_per_group": info["blobs_per_group"],
                       "groups": info["groups"], "group_bytes": info["group_bytes"], "batched": info["batched"], "inverse": info["inverse"], "forward": info["forward"]}
                rows.append(row)
                print(json.dumps(row), flush=True)
            srs.drop_multiproof()
    srs.close()
    if single_only:
        plib.kzg_srs_free(psrs)

for s in skipped:
    print("skipped (outputs over ENCB_MAX_OUT_BYTES): " + json.dumps(s), flush=True)
if os.environ.get("ENCB_OUT"):                                                                 # all rows as one JSON file
    with open(os.environ["ENCB_OUT"], "w") as f:
        json.dump(rows, f, indent=1)
