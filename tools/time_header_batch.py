#!/usr/bin/env python3
"""Times batched header verification on one GPU and writes profiles/header_batch.md.

    python tools/time_header_batch.py [--resources REMARKS.txt] [--out profiles/header_batch.md]

Measured, medians of 7 runs after 2 warm-ups with min and max, all in ONE run:
  * kzg_verify_length_proof_batch at count = 64, 1 024, 4 096, 65 536 with 4 claimed lengths, derived weights;
  * beside it the loop of kzg_verify_length_proof over 64 of those headers, scaled by count: what the batch is measured against;
  * kzg_g2_check_subgroup of 2 count points alone, beside 256 host kzg_validate_g2_point calls scaled up;
  * the split of the batch call by its KZG_VB_TRACE phases.
Headers come from a known tau (N = 1024); a pool of 1 024 distinct headers is tiled up to the count (equal headers cost what distinct
ones cost: every lane runs the same trip count).  --resources: the compiler's remarks for g2batch.hip
(make -C rust-kzg-bn254_amd/csrc -B g2batch.o EXTRA=-Rpass-analysis=kernel-resource-usage 2> REMARKS.txt), turned into the register table.
"""
import argparse
import ctypes as C
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
COUNTS = (64, 1024, 4096, 65536)
RUNS, WARM = 7, 2


NOTES = ["", "## Reading the tables", "",
         "* Both kernels run one wave per SIMD (`amdgpu_waves_per_eu(1, 1)`): an XYZZ accumulator is 72 registers, the base point 36, and the",
         "  subgroup test holds two accumulators.  The VGPR spills of `k_g2_subgroup_check` are copies to AGPRs (`v_accvgpr_write` / `_read` of",
         "  a106-a109), placed in front of the chain loop and between the chain and the four closing additions: no spill goes to scratch and none",
         "  sits inside a doubling or an addition.  The scratch bytes are the frames of the out-of-line `g2_add_call` / `g2_dbl` / `g2_dbl_affine`",
         "  (operands passed by reference), as in `k_g2_mul_generator` (profiles/g2msm.md).",
         "* The device phases are latency-bound chains, not throughput-bound: 65 536 lanes (256 CUs x 4 SIMDs x one wave of 64) run at once, so",
         "  the subgroup phase and the weighted sums cost the same from 64 to 4 096 headers (two points each) and grow in steps of 65 536 lanes",
         "  beyond.  A chain step (one doubling, or one checked mixed addition) is about 15 us of dependent integer work at this occupancy; the",
         "  weighted chain is 128 doublings and, per wave, nearly 128 additions (the lanes' bits differ), then the 6 additions of the shuffle tree.",
         "* The loop of single calls is two pairing checks per header (four Miller loops, two final exponentiations) on the host; the batch pays",
         "  2 + (non-empty groups) Miller loops on the host pool and one final exponentiation whatever the count."]


def timed(fn):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(RUNS):
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
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", text, re.S):
        name = re.search(r"k_g2_\w+?(?=E[PK])", m.group(1))
        if not name or "g2batch.hip" not in text[text.rfind("\n", 0, m.start()) + 1:m.start()]:
            continue
        body = m.group(2)
        get = lambda key: re.search(re.escape(key) + r": (\d+)", body).group(1)   # noqa: E731
        rows.append((name.group(0), get("VGPRs"), get("AGPRs"), get("VGPRs Spill"), get("SGPRs Spill"), get("ScratchSize [bytes/lane]"), get("Occupancy [waves/SIMD]"), m.group(3)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "header_batch.md"))
    ap.add_argument("--counts", default=",".join(str(c) for c in COUNTS))
    a = ap.parse_args()
    counts = [int(c) for c in a.counts.split(",")]
    k.load()
    L = k._lib
    ctx = L.Context(0)
    rnd = random.Random(11)
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

    # the single-call loop over 64 headers, and 256 host subgroup tests
    def loop64():
        for i in range(64):
            assert k.verifier.verify_length_proof(c[i], c2[i], pi2[i], shifts[lens[i]])
    loop = timed(loop64)
    reason = L.i32(0)
    pts256 = [np.ascontiguousarray(p) for p in np.concatenate([c2[:128], pi2[:128]])]

    def host256():
        for p in pts256:
            L.load().kzg_validate_g2_point(L.ptr(p), C.byref(reason))
    host_sub = timed(host256)

    rows, sub_rows, phase_rows = [], [], []
    for count in counts:
        reps = (count + POOL - 1) // POOL
        cc, cc2, cpi2 = (np.tile(x, (reps, 1))[:count] for x in (c, c2, pi2))
        clens = (lens * reps)[:count]

        def run():
            assert k.verifier.verify_length_proof_batch(cc, cc2, cpi2, clens, shifts, ctx=ctx)
        b = timed(run)
        rows.append((count, b, tuple(t * count / 64 for t in loop)))
        trace = captured_stderr(run)
        m = re.search(r"on-twist ([\d.]+) ms, subgroup ([\d.]+) ms, weights \+ weighted sums ([\d.]+) ms, G1 MSM ([\d.]+) ms, host sums \+ pairing ([\d.]+) ms", trace)
        phase_rows.append((count,) + tuple(float(v) for v in m.groups()) if m else (count,))
        pts = np.ascontiguousarray(np.concatenate([cc2, cpi2]))
        s = timed(lambda: k.helpers.check_g2_subgroup(pts, ctx=ctx))
        sub_rows.append((count, s, tuple(t * 2 * count / 256 for t in host_sub)))

    f3 = lambda t: "%.3f (%.3f - %.3f)" % t                                      # noqa: E731
    out = ["# Batched header verification: `kzg_verify_length_proof_batch`, `kzg_g2_check_subgroup`", "",
           "Written by `tools/time_header_batch.py` from one run on one MI355X.  Times in ms: median of %d runs after %d warm-ups (min - max)." % (RUNS, WARM),
           "Headers: known tau, N = 1024, claimed lengths drawn from {1, 4, 64, 1024}, a pool of 1 024 distinct headers tiled up to the count.", "",
           "## Register budgets (hipcc -O3 --offload-arch=gfx950, `-Rpass-analysis=kernel-resource-usage`)", "",
           "| kernel | VGPRs | AGPRs | VGPR spills | SGPR spills | scratch B/lane | waves/SIMD | LDS B/block |", "|---|---|---|---|---|---|---|---|"]
    res = resource_table(a.resources)
    out += ["| `%s` | %s | %s | %s | %s | %s | %s | %s |" % r for r in res] or ["| (no remarks file given) | | | | | | | |"]
    out += ["", "## The batch against the loop of single calls (same run)", "",
            "| count | batch | 64 single calls scaled to count | loop / batch |", "|---|---|---|---|"]
    out += ["| %d | %s | %s | %.1f x |" % (n, f3(b), f3(l), l[0] / b[0]) for n, b, l in rows]
    out += ["", "## The subgroup test alone: device chain against the host's [r]P", "",
            "| points | `kzg_g2_check_subgroup` | 256 `kzg_validate_g2_point` scaled to the points | host / device |", "|---|---|---|---|"]
    out += ["| %d | %s | %s | %.1f x |" % (2 * n, f3(s), f3(h), h[0] / s[0]) for n, s, h in sub_rows]
    out += ["", "## Phases of one batch call (`KZG_VB_TRACE=1`, one call after the timed ones)", "",
            "| count | checks + upload + on-twist | subgroup | weights + weighted sums | G1 MSM | host sums + pairing |", "|---|---|---|---|---|---|"]
    out += ["| %d | %s |" % (r[0], " | ".join("%.3f" % v for v in r[1:]) if len(r) > 1 else "(no trace line)") for r in phase_rows]
    out += NOTES
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
