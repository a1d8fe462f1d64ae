#!/usr/bin/env python3
"""Times locating the bad headers of a batch on one GPU and writes profiles/header_locate.md and .json.

    python tools/time_header_locate.py [--resources REMARKS.txt] [--out profiles/header_locate.md]

Measured, all in ONE run, per shape (64, 1 024, 4 096 headers with one group per header; 65 536 headers in 1 024 groups of 64) and per
number of bad headers b = 0, 1, 8:
  * verifier.locate_bad_headers (kzg_verify_length_proof_batch_locate): median of 5 calls after 1 warm-up with min and max, the pairing
    checks it made, and its KZG_VB_TRACE phases from one more call (shared prefix, G2 group sums, G1 group sums, host sums, search);
  * the plain reject: verifier.verify_length_proof_batch on the same inputs;
  * the baseline this entry replaces: a bisection over verify_length_proof_batch written here (the same tree walk as the library's
    search: the root, then the left half of every failing range, the right half untested when the left holds), every pass a full call of
    the batch entry on the range's headers: median of 3 runs, and its number of passes.
Headers come from a known tau (N = 1024); a pool of 1 024 distinct headers is tiled up to the count; a bad header carries the length
proof of another pool header.  Weights are derived (the library's transcript) everywhere.  --resources: the compiler's remarks for
g2batch.hip and multilocate.hip
(make -C rust-kzg-bn254_amd/csrc -B g2batch.o multilocate.o EXTRA=-Rpass-analysis=kernel-resource-usage 2> REMARKS.txt), turned into
the register table of the new kernels: recorded, not asserted.
"""
import argparse
import json
import os
import random
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ["KZG_VB_TRACE"] = "1"                                   # read once, when the library loads

import numpy as np  # noqa: E402

try:
    import torch  # noqa: F401,E402  (load order, as tests/conftest.py)
except ImportError:
    pass
import pyref  # noqa: E402
from pyref import R_  # noqa: E402
import rust_kzg_bn254_amd as k  # noqa: E402

N = 1024
LENS = (1, 4, 64, 1024)
POOL = 1024
SHAPES = ((64, None), (1024, None), (4096, None), (65536, 64))      # (headers, headers per group; None: one group per header)
BAD = (0, 1, 8)
RUNS, WARM, BISECT_RUNS = 5, 1, 3
KERNELS = r"(k_g2_locate_terms|k_g2_locate_fold|k_locate_termsILi1E|k_locate_foldILi1E|k_locate_termsILi2E|k_locate_foldILi2E)"


def timed(fn, runs=RUNS, warm=WARM):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def captured_stderr(fn):
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def resource_table(path):
    rows = []
    if not path or not os.path.exists(path):
        return rows
    text = open(path, errors="replace").read()
    seen = set()
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", text, re.S):
        name = re.search(KERNELS, m.group(1))
        if not name or name.group(1) in seen:
            continue
        seen.add(name.group(1))
        body = m.group(2)
        get = lambda key: re.search(re.escape(key) + r": (\d+)", body).group(1)   # noqa: E731
        shown = re.sub(r"ILi(\d)E", r"<\1>", name.group(1))
        rows.append((shown, get("VGPRs"), get("AGPRs"), get("VGPRs Spill"), get("SGPRs Spill"), get("ScratchSize [bytes/lane]"), get("Occupancy [waves/SIMD]"), m.group(3)))
    return rows


def bisect(batch_ok, n_units):
    """the bad units among n_units by passes of batch_ok(lo, hi) over unit ranges: (bad units, passes)"""
    passes, bad = 0, []
    stack = [(0, n_units, False)]
    while stack:
        lo, hi, fails = stack.pop()
        if not fails:
            passes += 1
            if batch_ok(lo, hi):
                continue
        if hi - lo == 1:
            bad.append(lo)
            continue
        mid = lo + (hi - lo) // 2
        passes += 1
        if batch_ok(lo, mid):
            stack.append((mid, hi, True))
        else:
            stack.append((mid, hi, False))
            stack.append((lo, mid, True))
    return sorted(bad), passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "header_locate.md"))
    a = ap.parse_args()
    k.load()
    ctx = k._lib.Context(0)
    rnd = random.Random(12)
    tau = rnd.randrange(2, R_)
    g1 = lambda s: pyref.point_to_wire(pyref.ec_mul(s % R_, (1, 2)))            # noqa: E731
    g2 = lambda s: k.helpers.g2_mul_generator(pyref.fr_to_mont(s % R_))         # noqa: E731
    shift_scalar = {d: pow(tau, N - d, R_) for d in LENS}
    shifts = {d: g1(s) for d, s in shift_scalar.items()}
    fs = [rnd.randrange(1, R_) for _ in range(POOL)]
    lens = [LENS[rnd.randrange(4)] for _ in range(POOL)]
    c = np.stack([g1(f) for f in fs])
    c2 = np.stack([g2(f) for f in fs])
    pi2 = np.stack([g2(shift_scalar[d] * f) for f, d in zip(fs, lens)])
    print("pool ready", flush=True)

    V = k.verifier
    rows = []
    for count, per_group in SHAPES:
        reps = (count + POOL - 1) // POOL
        cc, cc2 = (np.ascontiguousarray(np.tile(x, (reps, 1))[:count]) for x in (c, c2))
        clens = (lens * reps)[:count]
        n_groups = count if per_group is None else count // per_group
        unit = 1 if per_group is None else per_group
        groups = "item" if per_group is None else [i // per_group for i in range(count)]
        for b in BAD:
            cpi2 = np.ascontiguousarray(np.tile(pi2, (reps, 1))[:count])
            bad_pos = sorted(random.Random(count + b).sample(range(count), b))
            for pos in bad_pos:
                cpi2[pos] = pi2[(pos + 1) % POOL]
            want = sorted({pos // unit for pos in bad_pos})
            result = {}

            def run_locate():
                result["good"], result["checks"] = V.locate_bad_headers(cc, cc2, cpi2, clens, shifts, ctx=ctx, groups=groups, n_groups=None if per_group is None else n_groups)
            t_locate = timed(run_locate)
            assert list(np.flatnonzero(~result["good"])) == want, (count, b)
            trace = captured_stderr(run_locate)
            m = re.search(r"shared prefix ([\d.]+) ms, G2 group sums ([\d.]+) ms, G1 group sums ([\d.]+) ms, host sums ([\d.]+) ms, search ([\d.]+) ms", trace)
            phases = [float(v) for v in m.groups()] if m else []
            t_reject = timed(lambda: V.verify_length_proof_batch(cc, cc2, cpi2, clens, shifts, ctx=ctx))

            def batch_ok(lo, hi):
                s = slice(lo * unit, hi * unit)
                return V.verify_length_proof_batch(cc[s], cc2[s], cpi2[s], clens[s], shifts, ctx=ctx)

            def run_bisect():
                result["bisect"] = bisect(batch_ok, n_groups)
            t_bisect = timed(run_bisect, runs=BISECT_RUNS, warm=0)
            assert result["bisect"][0] == want, (count, b)
            rows.append({"headers": count, "groups": n_groups, "bad": b, "locate_ms": t_locate, "checks": result["checks"], "phases_ms": phases,
                         "reject_ms": t_reject, "bisect_ms": t_bisect, "bisect_passes": result["bisect"][1]})
            print("done", count, n_groups, b, "%.3f" % t_locate[0], result["checks"], "%.3f" % t_bisect[0], result["bisect"][1], flush=True)

    f3 = lambda t: "%.3f (%.3f - %.3f)" % tuple(t)                               # noqa: E731
    res = resource_table(a.resources)
    out = ["# Locating the bad headers of a batch: `kzg_verify_length_proof_batch_locate`", "",
           "Written by `tools/time_header_locate.py` from one run on one MI355X.  Times in ms: median (min - max) of %d calls after %d warm-up for the" % (RUNS, WARM),
           "library's entries, of %d runs for the bisection.  Headers: known tau, N = 1024, claimed lengths drawn from {1, 4, 64, 1024}, a pool of" % BISECT_RUNS,
           "1 024 distinct headers tiled up to the count; a bad header carries another header's length proof; derived weights everywhere.", "",
           "## Register budgets of the new G2 kernels and of both instantiations of the G1 pair (hipcc -O3 --offload-arch=gfx950, `-Rpass-analysis=kernel-resource-usage`; recorded, not asserted)", "",
           "| kernel | VGPRs | AGPRs | VGPR spills | SGPR spills | scratch B/lane | waves/SIMD | LDS B/block |", "|---|---|---|---|---|---|---|---|"]
    out += ["| `%s` | %s | %s | %s | %s | %s | %s | %s |" % r for r in res] or ["| (no remarks file given) | | | | | | | |"]
    out += ["", "## Locate against the bisection over `kzg_verify_length_proof_batch` (same run)", "",
            "| headers | groups | bad | locate | pairing checks | plain reject (one batch call) | bisection | passes | bisection / locate |", "|---|---|---|---|---|---|---|---|---|"]
    out += ["| %d | %d | %d | %s | %d | %s | %s | %d | %.1f x |" % (r["headers"], r["groups"], r["bad"], f3(r["locate_ms"]), r["checks"], f3(r["reject_ms"]), f3(r["bisect_ms"]),
                                                                 r["bisect_passes"], r["bisect_ms"][0] / r["locate_ms"][0]) for r in rows]
    out += ["", "## Phases of one locate call (`KZG_VB_TRACE=1`, one call after the timed ones)", "",
            "| headers | groups | bad | shared prefix | G2 group sums | G1 group sums | host sums | search |", "|---|---|---|---|---|---|---|---|"]
    out += ["| %d | %d | %d | %s |" % (r["headers"], r["groups"], r["bad"], " | ".join("%.3f" % v for v in r["phases_ms"]) if r["phases_ms"] else "(no trace line)") for r in rows]
    out += ["", "## Reading the tables", "",
            "* `shared prefix` is what the batch entry pays too: checks, upload, the on-twist and subgroup tests, the weights.  `G2 group sums` is the",
            "  segmented form of the batch entry's weighted sums (one chain per G2 point, then the scan and the fold); `G1 group sums` is one GLV",
            "  multiplication per commitment with its scan and fold, and the upload of the commitments.",
            "* `host sums` is the assembly of the leaves and their prefix sums in group order: linear in groups x (2 + lengths present), one",
            "  thread.  `search` is the pairing checks alone: 3 + (lengths present) Miller loops on the host pool and one final exponentiation each,",
            "  rho on the G1 side.",
            "* A bisection pass is a whole call of the batch entry on the range's headers: its subgroup test and its 128-step chains again, and a",
            "  transcript of the range.  With b = 0 the bisection is the one accepting call, and locate costs the group sums on top of it: call",
            "  the batch entry first and this entry after a reject."]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    with open(os.path.splitext(a.out)[0] + ".json", "w") as f:
        json.dump({"runs": RUNS, "warm": WARM, "bisect_runs": BISECT_RUNS, "resources": [list(r) for r in res], "rows": rows}, f, indent=1)
        f.write("\n")
    print(text)


if __name__ == "__main__":
    main()
