"""Per-blob time of KZG.recover_from_cosets_batch (`kzg_recover_from_cosets_batch`) next to the loop of KZG.recover_from_cosets calls over
the same blobs, in the same run on the same device, from host buffers to host arrays (every timed window ends in the call's own device
synchronisation).  Shapes: (n = 2^13, l = 1) and (2^16, 64) with half of the cosets missing at B = 1, 4, 16, 64, and (2^20, 16) with one
coset missing at B <= 16; each once with ONE index row for all blobs (one pattern) and once with a row per blob and B distinct missing
sets.  The values are random field elements (a call interpolates whatever it is given); the batch's rows are compared with the loop's bit
for bit before anything is timed.  Both are the Python surface, which allocates every result (the loop keeps its B results alive, as a
caller would); the same pair is timed once more at the C-ABI into arrays allocated once (`abi_*`), which leaves out numpy's allocations and
the polynomial wrappers.  Each measurement: two warm-ups, then the median of RB_REPS (9) with min and max, in ms per blob.
RB_SHAPES="log_n:l:missing:maxB,..." (missing = half | one) overrides the shapes, RB_BLOBS the batch sizes, RB_OUT names a JSON file."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (load order: see tests/conftest.py)
import rust_kzg_bn254_amd as k
from rust_kzg_bn254_amd import _lib

lib = _lib.load()

ctx = k.Context(0)
kz = k.KZG.new(ctx)
shapes = [s.split(":") for s in os.environ.get("RB_SHAPES", "13:1:half:64,16:64:half:64,20:16:one:16").split(",")]
batch_sizes = [int(b) for b in os.environ.get("RB_BLOBS", "1,4,16,64").split(",")]
reps = int(os.environ.get("RB_REPS", "9"))
rows = []


def per_blob_ms(fn, blobs):
    for _ in range(2):                                                                        # warm-up: tables, workspaces, code objects
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3 / blobs)
    return round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)


for log_n, l, missing, max_b in shapes:
    n, l, max_b = 1 << int(log_n), int(l), int(max_b)
    m = n // l
    count = m // 2 if missing == "half" else m - 1
    rng = np.random.Generator(np.random.PCG64(n + l))
    for B in [b for b in batch_sizes if b <= max_b]:
        ys = rng.integers(0, 1 << 60, size=(B, count, l, 4), dtype=np.uint64)                 # < 2^252: canonical wire words
        for patterns in ("shared", "distinct"):
            if patterns == "shared":
                idx = np.arange(0, m, 2, dtype=np.uint64) if missing == "half" else np.arange(0, m - 1, dtype=np.uint64)
                row_of = lambda b: idx
            else:                                                                             # blob b: its own random half / its own missing coset
                idx = np.stack([np.sort(rng.permutation(m)[:count]) if missing == "half" else np.delete(np.arange(m), (b * 7919) % m)
                                for b in range(B)]).astype(np.uint64)
                assert len({r.tobytes() for r in idx}) == B
                row_of = lambda b: idx[b]

            def loop():
                return [kz.recover_from_cosets(row_of(b), ys[b], n) for b in range(B)]

            def batch():
                return kz.recover_from_cosets_batch(idx, ys, n)

            out = np.zeros((B, n, 4), dtype=np.uint64)                                        # the C-ABI pair: outputs allocated (and touched) once
            flags = np.zeros(B, dtype=np.int32)
            flag = C.c_int32(0)

            def abi_loop():
                for b in range(B):
                    r = np.ascontiguousarray(row_of(b))
                    assert lib.kzg_recover_from_cosets(ctx.handle, _lib.ptr(ys[b]), _lib.ptr(r), count, n, l, 0, 1, _lib.ptr(out[b]), C.byref(flag)) == 0

            def abi_batch():
                assert lib.kzg_recover_from_cosets_batch(ctx.handle, _lib.ptr(ys), _lib.ptr(idx), 1 if idx.ndim == 1 else B, B, count, n, l, 0, 1, 0, _lib.ptr(out),
                                                         flags.ctypes.data_as(C.POINTER(C.c_int32))) == 0

            got, consistent = batch()
            same = bool(consistent.all()) and all(np.array_equal(got[b], p.evaluations()) for b, p in enumerate(loop()))
            del got
            t_loop, t_batch = per_blob_ms(loop, B), per_blob_ms(batch, B)
            a_loop, a_batch = per_blob_ms(abi_loop, B), per_blob_ms(abi_batch, B)
            info = k.helpers.recover_batch_info(B, count, n, l)
            row = {"n": n, "chunk_len": l, "m": m, "missing": m - count, "blobs": B, "patterns": patterns, "batch_equals_loop": same,
                   "loop_ms_per_blob": t_loop[0], "loop_min": t_loop[1], "loop_max": t_loop[2],
                   "batch_ms_per_blob": t_batch[0], "batch_min": t_batch[1], "batch_max": t_batch[2],
                   "loop_over_batch": round(t_loop[0] / t_batch[0], 2),
                   "abi_loop_ms_per_blob": a_loop[0], "abi_loop_min": a_loop[1], "abi_loop_max": a_loop[2],
                   "abi_batch_ms_per_blob": a_batch[0], "abi_batch_min": a_batch[1], "abi_batch_max": a_batch[2],
                   "abi_loop_over_batch": round(a_loop[0] / a_batch[0], 2), "groups": info["groups"], "reps": reps}
            rows.append(row)
            print(json.dumps(row), flush=True)
            assert same, "the batch's rows differ from the loop's"

if os.environ.get("RB_OUT"):                                                                   # all rows as one JSON file
    with open(os.environ["RB_OUT"], "w") as f:
        json.dump(rows, f, indent=1)
