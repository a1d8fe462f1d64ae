#!/usr/bin/env python3
"""Times the batched prover against the routes that existed before it, from host buffers, on one GPU.

For every n in --ns and count in --counts (seeded random polynomials / blobs, random points):
  proofs   KZG.compute_proof_batch                   | a loop of kzg_compute_proof | kzg_compute_proof_begin / _end, three in flight
  blobs    KZG.commit_and_prove_blob_batch           | a loop of kzg_commit_and_prove_blob | the blob stream, three in flight
Every call ends in a device synchronise inside the library (results are on the host when it returns), so a host clock around the call is
the call's time.  Each shape is warmed once per route; the routes are then timed alternately --reps times and the median, minimum and
maximum are kept.  The batch results are compared with the single calls' on the first and last rows of every shape.

--baselines leaves the batch routes out: that is how a build of the parent commit (KZG_LIB_PATH=<its library>) is timed in the same
session.  --batch-only times the two batch routes alone.  --trace runs one batch call per shape and nothing else: with KZG_VB_TRACE=1 in the environment the library prints where the
time of that call goes (pack + upload + transcripts / commitments / fused kernel / MSM) on stderr.

Writes one JSON document (--out) and a table on stdout.  Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW = ("kzg_compute_proof_batch", "kzg_compute_proof_batch_device", "kzg_compute_blob_proof_batch", "kzg_commit_and_prove_blob_batch",
       "kzg_ctx_set_prove_group_bytes")
TAU = 0x1234567890ABCDEF1234567890ABCDEF


def wire_rows(rng, rows):
    """rows x 4 words, every element below 2^252 < r: valid wire elements"""
    a = rng.integers(0, 1 << 63, size=(rows, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="512,1024,2048,4096")
    ap.add_argument("--counts", default="1,16,256,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baselines", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--batch-only", action="store_true", help="time the two batch routes alone (the comparison of results with the single calls stays)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ns = [int(v) for v in args.ns.split(",")]
    counts = [int(v) for v in args.counts.split(",")]

    from rust_kzg_bn254_amd import _lib as L
    if args.baselines:
        for name in NEW:
            L.PROTOTYPES.pop(name, None)
    import rust_kzg_bn254_amd as k
    lib = k.load()
    ctx = k.default_context()
    srs = k.SRS.generate(TAU, max(ns))
    kzg = k.KZG.new(ctx)
    rng = np.random.default_rng(20240607)
    results = []

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    for n in ns:
        srs.cache_lagrange(n)
        for count in counts:
            evals = wire_rows(rng, count * n).reshape(count, n, 4)
            zs = wire_rows(rng, count)
            blobs_np = rng.integers(0, 256, size=(count, n * 32), dtype=np.uint8)
            blobs_np[:, ::32] = 0                                                         # canonical elements, as Blob::new demands
            blobs = [k.Blob.from_padded_unchecked(blobs_np[b].tobytes()) for b in range(count)]
            out = np.zeros((count, 8), np.uint64); ys = np.zeros((count, 4), np.uint64); inf = np.zeros(count, np.uint8)
            com = np.zeros((count, 8), np.uint64); zz = np.zeros((count, 4), np.uint64); cinf = np.zeros(count, np.uint8)
            ev_p = [evals[b].ctypes.data_as(L.u64p) for b in range(count)]
            z_p = [zs[b].ctypes.data_as(L.u64p) for b in range(count)]
            o_p = [out[b].ctypes.data_as(L.u64p) for b in range(count)]
            y_p = [ys[b].ctypes.data_as(L.u64p) for b in range(count)]
            i_p = [inf[b:].ctypes.data_as(L.u8p) for b in range(count)]
            c_p = [com[b].ctypes.data_as(L.u64p) for b in range(count)]
            zz_p = [zz[b].ctypes.data_as(L.u64p) for b in range(count)]
            ci_p = [cinf[b:].ctypes.data_as(L.u8p) for b in range(count)]
            b_p = [blobs_np[b].ctypes.data_as(L.u8p) for b in range(count)]
            blen = n * 32

            def ok(rc):
                if rc != L.OK:
                    raise RuntimeError("status %d: %s" % (rc, ctx.last_error()))

            def proofs_loop():
                for b in range(count):
                    ok(lib.kzg_compute_proof(ctx.handle, srs.handle, ev_p[b], n, None, n, z_p[b], o_p[b], i_p[b], y_p[b]))

            def proofs_stream(depth=3):
                for b in range(count + depth):
                    if b >= depth:
                        ok(lib.kzg_compute_proof_end(ctx.handle, (b - depth) % depth, o_p[b - depth], i_p[b - depth], y_p[b - depth]))
                    if b < count:
                        ok(lib.kzg_compute_proof_begin(ctx.handle, srs.handle, ev_p[b], n, None, n, z_p[b], b % depth))

            def blobs_loop():
                for b in range(count):
                    ok(lib.kzg_commit_and_prove_blob(ctx.handle, srs.handle, b_p[b], blen, n, c_p[b], ci_p[b], o_p[b], i_p[b], zz_p[b], y_p[b]))

            def blobs_stream(depth=3):
                for b in range(count + depth):
                    if b >= depth:
                        ok(lib.kzg_commit_and_prove_blob_end(ctx.handle, (b - depth) % depth, c_p[b - depth], ci_p[b - depth], o_p[b - depth], i_p[b - depth],
                                                             zz_p[b - depth], y_p[b - depth]))
                    if b < count:
                        ok(lib.kzg_commit_and_prove_blob_begin(ctx.handle, srs.handle, b_p[b], blen, n, None, b % depth))

            got = {}

            def proofs_batch():
                got["p"] = kzg.compute_proof_batch(evals, zs, srs, want_y=True)

            def blobs_batch():
                got["b"] = kzg.commit_and_prove_blob_batch(blobs, srs)

            if args.trace:
                print("== n=%d count=%d" % (n, count), file=sys.stderr, flush=True)
                proofs_batch(); blobs_batch()                                             # warm
                print("-- compute_proof_batch", file=sys.stderr, flush=True)
                proofs_batch()
                print("-- commit_and_prove_blob_batch", file=sys.stderr, flush=True)
                blobs_batch()
                continue
            routes = [("proofs_loop", proofs_loop), ("proofs_stream3", proofs_stream), ("blobs_loop", blobs_loop), ("blobs_stream3", blobs_stream)]
            if args.batch_only:
                routes = []
            if not args.baselines:
                routes += [("proofs_batch", proofs_batch), ("blobs_batch", blobs_batch)]
            for _, fn in routes:
                fn()                                                                      # warm every route at this shape
            if not args.baselines:                                                        # same results: first and last row
                proofs_loop()
                for b in (0, count - 1):
                    assert np.array_equal(got["p"][0][b], out[b]) and np.array_equal(got["p"][1][b], ys[b]), (n, count, b)
                blobs_loop()
                for b in (0, count - 1):
                    assert np.array_equal(got["b"][0][b], com[b]) and np.array_equal(got["b"][1][b], out[b]), (n, count, b)
            times = {name: [] for name, _ in routes}
            for _ in range(args.reps):
                for name, fn in routes:
                    times[name].append(timed(fn))
            row = {"n": n, "count": count}
            for name, v in times.items():
                row[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
            results.append(row)
            print("n=%5d count=%5d  " % (n, count) + "  ".join("%s %.3f [%.3f, %.3f]" % (name, row[name]["median_ms"], row[name]["min_ms"], row[name]["max_ms"])
                                                           for name, _ in routes), flush=True)
    if args.out and not args.trace:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"library": L.LIB_PATH, "reps": args.reps, "unit": "ms per call of `count` items", "rows": results}, f, indent=1)
    srs.close()


if __name__ == "__main__":
    main()
