"""Per-blob time of the batched blob header (`kzg_commit_with_length_proof_batch`: the G1 commitments of the batched commitments, both G2
MSMs of a group of blobs in one sort and one launch sequence, csrc/g2msm.hip) on one MI355X, and beside it, in the same process, the loop
of B calls of `kzg_commit_with_length_proof` over the same blobs.  d = n in {2^12, 2^14, 2^16}, B in {1, 4, 16, 64}, setup order N = 2^16
(2^20 for d = 2^16).  Every timed window is one synchronous call (or the loop of B of them) from host buffers that returns host data; each
shape is warmed up twice; the figure is the median of the repetitions (min and max beside it).  The outputs of the two are compared bit for
bit in the run.  Writes <HCB_OUT>/header_commit_batch.json and .md (HCB_OUT defaults to profiles/); HCB_SIZES="12,14,16", HCB_BATCHES and
HCB_REPS override the shapes and the repetitions.  `--render FILE.json` writes the .md of a recorded run beside it (no GPU)."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAU = 0x1D2C3B4A5968778695A4B3C2D1E0F1234567


def timed_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def measure(sizes, batches, reps):
    import numpy as np
    import rust_kzg_bn254_amd as k
    from rust_kzg_bn254_amd import _lib, helpers
    lib = _lib.load()
    ctx = k.Context(0)
    out = {"reps": reps, "warmups": 2, "rows": []}
    rng = np.random.Generator(np.random.PCG64(11))
    for lg in sizes:
        d = n = 1 << lg
        N = 1 << 20 if lg >= 16 else 1 << 16
        g1 = k.SRS.generate(TAU, d, ctx=ctx)
        g2 = k.G2SRS.generate(TAU, d, ctx=ctx)
        trailing = k.G2SRS.generate(TAU, d, first_power=N - d, ctx=ctx)
        for B in batches:
            sc = np.ascontiguousarray(rng.integers(0, 1 << 60, size=(B, n, 4), dtype=np.uint64))      # < 2^252: canonical wire words
            c = np.zeros((B, 8), np.uint64); c2 = np.zeros((B, 16), np.uint64); pi2 = np.zeros((B, 16), np.uint64)
            lc = np.zeros((B, 8), np.uint64); lc2 = np.zeros((B, 16), np.uint64); lpi2 = np.zeros((B, 16), np.uint64)

            def batched():
                assert lib.kzg_commit_with_length_proof_batch(ctx.handle, g1.handle, g2.handle, trailing.handle, N - d, N, _lib.ptr(sc), n, B, d, _lib.ptr(c),
                                                              _lib.ptr(c2), _lib.ptr(pi2)) == 0

            def loop():
                for b in range(B):
                    assert lib.kzg_commit_with_length_proof(ctx.handle, g1.handle, g2.handle, trailing.handle, N - d, N, _lib.ptr(sc[b]), n, d, _lib.ptr(lc[b]),
                                                            _lib.ptr(lc2[b]), _lib.ptr(lpi2[b])) == 0

            for _ in range(2):
                batched(); loop()
            equal = bool(np.array_equal(c, lc) and np.array_equal(c2, lc2) and np.array_equal(pi2, lpi2))
            assert equal, (n, B)
            bt, lt = timed_ms(batched, reps), timed_ms(loop, reps)
            row = {"n": n, "srs_order": N, "blobs": B, "bit_equal": equal,
                   "batch_ms_per_blob": round(bt[0] / B, 4), "batch_min_ms_per_blob": round(bt[1] / B, 4), "batch_max_ms_per_blob": round(bt[2] / B, 4),
                   "loop_ms_per_blob": round(lt[0] / B, 4), "loop_min_ms_per_blob": round(lt[1] / B, 4), "loop_max_ms_per_blob": round(lt[2] / B, 4),
                   "loop_over_batch": round(lt[0] / bt[0], 2), "plan": helpers.g2_batch_info(n, 2, B)}
            out["rows"].append(row)
            print({kk: v for kk, v in row.items() if kk != "plan"}, flush=True)
        for h in (g1, g2, trailing):
            h.close()
    return out


def render(out, path):
    with open(path, "w") as f:
        f.write("# Blob headers for many blobs in one call: measured per-blob times\n\n")
        f.write("Written by `tools/time_header_commit_batch.py` on one MI355X (`header_commit_batch.json` holds the same rows and the plan of every\n"
                "shape).  `batch`: one call of `kzg_commit_with_length_proof_batch` over B blobs of n = d coefficients; `loop`: B calls of\n"
                "`kzg_commit_with_length_proof` over the same blobs, in the same process.  Synchronous calls from host buffers, 2 warm-ups, median of\n"
                "%d repetitions with minimum and maximum, all in milliseconds PER BLOB.  The outputs of the two were compared bit for bit in the run.\n"
                "Plan columns (`helpers.g2_batch_info`, a full group): blobs per group x groups, buckets G of one base set, accumulate lanes nl,\n"
                "sorted entries per lane seg, sort form, scan form, launches per group.\n\n" % out["reps"])
        f.write("| n = d | N | B | batch median (min .. max) | loop median (min .. max) | loop / batch | group x groups | G | nl | seg | sort | scan | launches |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in out["rows"]:
            p = r["plan"]
            f.write("| 2^%d | 2^%d | %d | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.2f | %d x %d | %d | %d | %d | %s | %s | %d |\n" % (
                r["n"].bit_length() - 1, r["srs_order"].bit_length() - 1, r["blobs"], r["batch_ms_per_blob"], r["batch_min_ms_per_blob"], r["batch_max_ms_per_blob"],
                r["loop_ms_per_blob"], r["loop_min_ms_per_blob"], r["loop_max_ms_per_blob"], r["loop_over_batch"], p["blobs_per_group"], p["groups"], p["G"], p["nl"],
                p["seg"], "small" if p["sort_small"] else "tiled", "one workgroup" if p["scan1"] else "three kernels", p["launches"]))
        # the condition of the change: for B >= 4 the batched call is no slower per blob than the loop, medians compared, the loop's own
        # min .. max spread as the margin
        judged = [r for r in out["rows"] if r["blobs"] >= 4]
        lost = [r for r in judged if r["batch_ms_per_blob"] > r["loop_ms_per_blob"] + (r["loop_max_ms_per_blob"] - r["loop_min_ms_per_blob"])]
        f.write("\nCondition (every shape with B >= 4: the batched median no slower per blob than the loop's median, the loop's own min .. max spread as the\n"
                "margin): %d of %d shapes hold" % (len(judged) - len(lost), len(judged)))
        if lost:
            f.write("; losing shapes: " + ", ".join("n = 2^%d B = %d" % (r["n"].bit_length() - 1, r["blobs"]) for r in lost))
        f.write(".  Every row is bit-equal: %s.\n" % ("yes" if all(r["bit_equal"] for r in out["rows"]) else "NO"))
        ones = [r for r in out["rows"] if r["blobs"] == 1]
        if ones:
            f.write("B = 1 takes the batched plan too (lanes capped at four per bucket) and is %s times faster than the single call, whose own plan is\n"
                    "left as it is in this change.\n" % ", ".join("%.1f" % r["loop_over_batch"] for r in ones))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--render":
        render(json.load(open(sys.argv[2])), os.path.splitext(sys.argv[2])[0] + ".md")
        sys.exit(0)
    sizes = [int(s) for s in os.environ.get("HCB_SIZES", "12,14,16").split(",")]
    batches = [int(s) for s in os.environ.get("HCB_BATCHES", "1,4,16,64").split(",")]
    out_dir = os.environ.get("HCB_OUT", os.path.join(ROOT, "profiles"))
    result = measure(sizes, batches, int(os.environ.get("HCB_REPS", "7")))
    os.makedirs(out_dir, exist_ok=True)
    json.dump(result, open(os.path.join(out_dir, "header_commit_batch.json"), "w"), indent=1)
    render(result, os.path.join(out_dir, "header_commit_batch.md"))
