#!/usr/bin/env python3
"""Times the two routes from a file of gnark-compressed G2 points to a device-resident G2 SRS on one GPU and writes
profiles/g2_decompress.md.

    python tools/g2_decompress_times.py [--resources REMARKS.txt] [--kernel-stats STATS.csv] [--out profiles/g2_decompress.md]
    python tools/g2_decompress_times.py --once 16        # one load and one kzg_g2_check_subgroup of 2^16 points: the workload of the
                                                          # rocprofv3 --kernel-trace --stats run whose CSV --kernel-stats reads

Measured box to box (host bytes in, resident handle out), medians of 5 runs after 1 warm-up with min and max, all in ONE run:
  * the device loader `kzg_g2srs_load_compressed_be` at n = 2^12, 2^16, 2^20;
  * the host route it replaces in `G2SRS.from_file`: `kzg_g2_decompress_be` on the host pool, then `kzg_g2srs_upload`, at 2^12 and 2^16
    (--host-log 20 adds 2^20: about a minute per run).
Inputs: [tau^(1 + i)]_2 of a known tau from `kzg_g2srs_generate`, compressed with Python integers (tests/g2_compress_ref.py); 2^16
distinct points, tiled for 2^20 (every lane runs the same trip counts whatever the point).  The host pool runs KZG_HOST_THREADS
threads, 16 unless the variable is set.  --resources: the compiler's remarks for g2decode.hip
(make -C rust-kzg-bn254_amd/csrc -B g2decode.o EXTRA=-Rpass-analysis=kernel-resource-usage 2> REMARKS.txt), turned into the register table.
"""
import argparse
import ctypes as C
import csv
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("KZG_HOST_THREADS", "16")                    # read once, when the library loads

import numpy as np  # noqa: E402

try:
    import torch  # noqa: F401,E402  (load order, as tests/conftest.py)
except ImportError:
    pass
import rust_kzg_bn254_amd as k  # noqa: E402
from pyref import P  # noqa: E402
from rust_kzg_bn254_amd import _lib, helpers  # noqa: E402

TAU = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CF
DISTINCT_LOG = 16
RUNS, WARM = 5, 1
RINV = pow(1 << 256, -1, P)
HALF = (P - 1) // 2

NOTES = ["## Reading the tables", "",
         "* Square root and subgroup chain are ONE kernel, not two over the same buffer: the fused kernel has no VGPR or SGPR spill, and its scratch and",
         "  LDS figures are those of `k_g2_subgroup_check` alone (profiles/header_batch.md: 256 VGPRs, 110 AGPRs, 1616 B/lane, 2304 B/block) -- the scratch",
         "  bytes are the frames of the out-of-line `g2_add_call` / `g2_dbl` / `g2_dbl_affine` of the chain, the table of a^1 .. a^7 of the square root",
         "  stays in registers (it is dead when the chain starts; 30 - 36 more AGPRs are all the fusion costs).  One wave per SIMD, as budgeted.",
         "* The kernel is a latency-bound chain per lane: 65 536 lanes (256 CUs x 4 SIMDs x one wave of 64) run at once, so 2^12 and 2^16 points cost",
         "  nearly the same, and 2^20 points are 16 launches of 65 536 behind chunked uploads (1 MiB chunks through the two halves of slot 0's pinned",
         "  result buffer; no pinned allocation grows with n).",
         "* The host route is `kzg_g2_decompress_be` on the pool (three exponentiations, one inversion and the 254-bit [r]P per point) plus",
         "  `kzg_g2srs_upload`; its time is proportional to n.  By proportion of its 2^12 figure it would meet the device loader's floor at about 140",
         "  points (not measured); `G2SRS.from_file` uses the device loader at every size: below that it gives away under 2 ms, once, and it is the",
         "  route that accepts the generator a file of powers of tau starts with."]


def compress(wire) -> bytes:
    """(n, 16) wire points -> gnark bytes; the arithmetic of tests/g2_compress_ref.py without the per-point objects"""
    rows = np.ascontiguousarray(wire, dtype=np.uint64).reshape(-1, 4, 4)
    out = bytearray(64 * len(rows))
    for i, r in enumerate(rows):
        x0, x1, y0, y1 = (int.from_bytes(r[j].tobytes(), "little") * RINV % P for j in range(4))
        out[64 * i:64 * i + 32] = x1.to_bytes(32, "big")
        out[64 * i + 32:64 * i + 64] = x0.to_bytes(32, "big")
        out[64 * i] |= 0xC0 if (y1 > HALF if y1 else y0 > HALF) else 0x80
    return bytes(out)


def timed(fn, runs=RUNS, warm=WARM):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def device_load(data):
    ctx = _lib.default_context()
    h = C.c_void_p()
    buf = np.frombuffer(data, dtype=np.uint8)
    rc = _lib.load().kzg_g2srs_load_compressed_be(ctx.handle, buf.ctypes.data_as(_lib.u8p), len(data) // 64, C.byref(h), None)
    assert rc == _lib.OK, rc
    return h


def host_route(data):
    ctx = _lib.default_context()
    n = len(data) // 64
    wire = np.zeros((n, 16), np.uint64)
    buf = np.frombuffer(data, dtype=np.uint8)
    assert _lib.load().kzg_g2_decompress_be(buf.ctypes.data_as(_lib.u8p), n, _lib.ptr(wire), None) == _lib.OK
    h = C.c_void_p()
    assert _lib.load().kzg_g2srs_upload(ctx.handle, _lib.ptr(wire), n, C.byref(h), None) == _lib.OK
    return h


def freeing(fn, data):
    def run():
        _lib.load().kzg_g2srs_free(fn(data))
    return run


def fmt(t):
    return "%.3f (%.3f - %.3f)" % t


def resource_table(path):
    text = open(path).read()
    rows = []
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", text, re.S):
        name, body, lds = m.group(1), m.group(2), m.group(3)
        if "k_g2_decompress" not in name:
            continue
        g = lambda key: re.search(re.escape(key) + r": (\d+)", body).group(1)      # noqa: E731
        label = "`k_g2_decompress<%s>`" % ("true" if "ILb1E" in name else "false")
        rows.append("| %s | %s | %s | %s | %s | %s | %s | %s |" % (label, g("VGPRs"), g("AGPRs"), g("VGPRs Spill"), g("SGPRs Spill"), g("ScratchSize [bytes/lane]"),
                                                                  g("Occupancy [waves/SIMD]"), lds))
    return ["## Register budgets (hipcc -O3 --offload-arch=gfx950, `-Rpass-analysis=kernel-resource-usage`)", "",
            "| kernel | VGPRs | AGPRs | VGPR spills | SGPR spills | scratch B/lane | waves/SIMD | LDS B/block |", "|---|---|---|---|---|---|---|---|"] + sorted(set(rows)) + [""]


def kernel_table(path):
    rows = []
    for r in csv.DictReader(open(path)):
        name = r.get("Name", "")
        if "k_g2_decompress" in name or "k_g2_subgroup_check" in name:
            short = "k_g2_decompress" if "k_g2_decompress" in name else "k_g2_subgroup_check"
            rows.append("| `%s` | %s | %.3f |" % (short, r["Calls"], float(r["AverageNs"]) / 1e6))
    return ["## Kernel times at 2^16 points (`rocprofv3 --kernel-trace --stats`, the run of `--once 16`)", "",
            "| kernel | calls | average ms |", "|---|---|---|"] + rows + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g2_decompress.md"))
    ap.add_argument("--resources")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--host-log", type=int, default=16, help="largest log2(n) of the host route")
    ap.add_argument("--once", type=int, help="one device load and one subgroup check of 2^ONCE points, nothing written")
    a = ap.parse_args()

    top = a.once if a.once is not None else DISTINCT_LOG
    srs = k.G2SRS.generate(TAU, 1 << min(top, DISTINCT_LOG), first_power=1)
    wire = srs.g2
    srs.close()
    distinct = compress(wire)
    if a.once is not None:
        data = distinct[:64 << a.once]
        _lib.load().kzg_g2srs_free(device_load(data))
        helpers.check_g2_subgroup(wire[:1 << a.once])
        print("loaded and checked 2^%d points" % a.once)
        return

    # the two routes give the same handle
    h1, h2 = device_load(distinct[:64 << 12]), host_route(distinct[:64 << 12])
    ctx = _lib.default_context()
    got = [k.G2SRS(h, 1 << 12, ctx) for h in (h1, h2)]
    assert np.array_equal(got[0].g2, wire[:1 << 12]) and np.array_equal(got[1].g2, wire[:1 << 12])
    for s in got:
        s.close()

    lines = ["# Compressed G2 points to a resident G2 SRS: device loader against the host route", "",
             "Written by `tools/g2_decompress_times.py` from one run on one MI355X.  Times in ms, box to box from host bytes to the resident handle:",
             "median of %d runs after %d warm-up (min - max).  Host pool: %s threads (`KZG_HOST_THREADS`)." % (RUNS, WARM, os.environ["KZG_HOST_THREADS"]), ""]
    if a.resources:
        lines += resource_table(a.resources)
    lines += ["## `kzg_g2srs_load_compressed_be` against `kzg_g2_decompress_be` + `kzg_g2srs_upload` (same run)", "",
              "| points | device loader | host route | host / device |", "|---|---|---|---|"]
    results = {}
    for log_n in (12, 16, 20):
        data = distinct[:64 << log_n] if log_n <= DISTINCT_LOG else distinct * (1 << (log_n - DISTINCT_LOG))
        dev = timed(freeing(device_load, data))
        host = timed(freeing(host_route, data)) if log_n <= a.host_log else None
        results[log_n] = (dev, host)
        lines.append("| 2^%d | %s | %s | %s |" % (log_n, fmt(dev), fmt(host) if host else "not run", "%.1f x" % (host[0] / dev[0]) if host else ""))
        print(lines[-1], flush=True)
    lines.append("")
    ok12, ok16 = results[12][0][0] <= results[12][1][0], results[16][0][0] < results[16][1][0]
    lines += ["## The crossover", "",
              "Required: the device loader not slower than the host route at 2^12 points and faster at 2^16.  Measured: 2^12 %s, 2^16 %s."
              % ("holds" if ok12 else "DOES NOT HOLD", "holds" if ok16 else "DOES NOT HOLD"), ""]
    if a.kernel_stats:
        lines += kernel_table(a.kernel_stats)
    lines += NOTES
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
