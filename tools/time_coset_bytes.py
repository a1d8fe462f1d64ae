"""Per-call time of verifying a batch of coset proofs that arrives as BYTES (32-byte gnark-compressed commitments and proofs, 32-byte
big-endian values), weights derived inside the call, rows (N, chunk_len) in (65536, 64), (65536, 16), (65536, 1), (4096, 16), (256, 16);
n = 2^16, items as tools/time_fs_device.py builds them.  Four variants, taken in turns inside one loop so that drift of the machine hits them
alike, one warm-up each, then CB_REPS (7) rounds; median, minimum and maximum per variant, host clock around calls that end synchronised:

  a  the PARENT commit's library (CB_BASELINE_LIB, its own context and SRS): kzg_verify_multiproof_batch on already decoded inputs
  b  this library: kzg_coset_items_decode_be, plus the commitments through kzg_g1_decompress_be_device, on its own
  c  this library: kzg_verify_multiproof_batch_bytes
  d  what a caller of the parent has to do today: proofs and commitments through kzg_srs_load_compressed_be + kzg_srs_download
     (KZG_NO_PRECOMPUTE=1 for those loads: no tables), values through the Python / numpy codec (fr.frs_from_ints), then a.  The codec
     takes seconds at 10^6 values, so rows with more than 2^16 values run d in CB_D_REPS (3) of the rounds only.

The fusion gate, rows (65536, 64) and (65536, 16): c <= (a + b) x 1.05.  c against d is reported, not gated.  A child process with
KZG_VB_TRACE=1 gives the phase split of a and c (the library then synchronises between phases): median per phase of five calls.

Modes: no argument = measure, write CB_OUT (default profiles/coset_bytes.json; keys other than "rows" of an existing file are kept) and
render profiles/coset_bytes.md beside it; --render = render only; --resources FILE = take the kernels' resource table from the output of
`hipcc -Rpass-analysis=kernel-resource-usage`; --kernel-stats FILE = take the decode kernels' rows from a rocprofv3 kernel_stats CSV;
--bench PARENT.json THIS.json = the bench.py headline of both libraries on one box.  CB_ROWS="N,l;N,l" restricts the rows,
CB_VARIANTS="b,c" the variants (a profiler run), CB_NO_TRACE=1 skips the child."""
import ctypes as C, csv, hashlib, json, os, re, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.environ.get("CB_OUT", os.path.join(ROOT, "profiles", "coset_bytes.json"))
KERNELS = ("k_g1_decode_be", "k_fr_decode_be", "k_coset_item_digests_bytes")
GATE_ROWS = ((65536, 64), (65536, 16))


def load_json():
    return json.load(open(OUT)) if os.path.exists(OUT) else {}


def save_json(doc):
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)


def fmt(cell):
    return "–" if not cell else "%.3f (%.3f – %.3f)" % (cell["median"], cell["min"], cell["max"])


def size(nbytes):
    return "%d MiB" % (nbytes >> 20) if nbytes >= 1 << 20 else "%d KiB" % (nbytes >> 10)


def render(doc):
    rows = doc.get("rows", [])
    L = ["# Coset-proof batches verified from serialized bytes (`g1_decode.h`, `cosetbytes.hip`, `kzg_verify_multiproof_batch_bytes`)", "",
         "Every figure is from one MI355X (`tools/time_coset_bytes.py`) and is in `coset_bytes.json` beside this file.  n = 2^16, weights derived inside",
         "the call, host buffers; the variants were taken in turns inside each round after one warm-up each.", "",
         "- **a** the parent commit's library, `kzg_verify_multiproof_batch` on already decoded inputs (same process, own context and SRS)",
         "- **b** this library, `kzg_coset_items_decode_be` plus the commitments through `kzg_g1_decompress_be_device`, on its own",
         "- **c** this library, `kzg_verify_multiproof_batch_bytes`",
         "- **d** a caller of the parent today: points through `kzg_srs_load_compressed_be` + `kzg_srs_download`, values through the Python codec, then a",
         "", "## Per call (ms: median, and min – max of the rounds)", "",
         "| N | l | values | a | b | c | d | rounds (d) | c / (a + b) | c / d |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        a, b, c, d = (r.get(v + "_ms") for v in "abcd")
        ratio = "%.3f" % (c["median"] / (a["median"] + b["median"])) if a and b and c else "–"
        cd = "%.4f" % (c["median"] / d["median"]) if c and d else "–"
        L.append("| %d | %d | %s | %s | %s | %s | %s | %s (%s) | %s | %s |" % (r["N"], r["chunk_len"], size(r["values_bytes"]), fmt(a), fmt(b), fmt(c), fmt(d),
                                                                          r.get("rounds", "–"), r.get("d_rounds", "–"), ratio, cd))
    gates = [r for r in rows if "gate_met" in r]
    if gates:
        L += ["", "**The fusion gate** (c ≤ (a + b) × 1.05): " + "  ".join(
            "(%d, %d): %.3f ≤ (%.3f + %.3f) × 1.05 = %.3f — %s." % (r["N"], r["chunk_len"], r["c_ms"]["median"], r["a_ms"]["median"], r["b_ms"]["median"],
                                                                      r["gate_bound_ms"], "met" if r["gate_met"] else "NOT met") for r in gates)]
    traced = [(r, v) for r in rows for v in "ac" if r.get(v + "_traced_phase_ms")]
    if traced:
        L += ["", "## Traced phases (KZG_VB_TRACE=1: synchronised between phases; median of 5 calls, ms)", ""]
        for r, v in traced:
            L.append("- (%d, %d) %s: " % (r["N"], r["chunk_len"], v) + ", ".join("%s %.3f" % kv for kv in r[v + "_traced_phase_ms"].items()))
    if doc.get("kernels"):
        L += ["", "## Kernels", "", "Compiler (`-Rpass-analysis=kernel-resource-usage`), gfx950.  `g1_decode.h` uses the 3-bit fixed window of `g2_decode.h`",
              "(`fq_sqrt_candidate`: a table of a^1 .. a^7, 249 squarings and at most 89 products per square root).", "",
              "| kernel | VGPRs | SGPRs | scratch | LDS | occupancy (waves / SIMD) |", "|---|---|---|---|---|---|"]
        for kk in doc["kernels"]:
            L.append("| `%s` | %d | %d | %d | %d | %d |" % (kk["kernel"], kk["vgprs"], kk["sgprs"], kk["scratch"], kk["lds"], kk["occupancy"]))
    if doc.get("kernel_trace"):
        kt = doc["kernel_trace"]
        L += ["", "One `rocprofv3 --kernel-trace --stats` run (no counters), %s:" % kt.get("what", ""), "",
              "| kernel | calls | total µs | average µs | min µs | max µs |", "|---|---|---|---|---|---|"]
        for s in kt["rows"]:
            L.append("| `%s` | %d | %.1f | %.1f | %.1f | %.1f |" % (s["kernel"], s["calls"], s["total_us"], s["avg_us"], s["min_us"], s["max_us"]))
    if doc.get("bench"):
        b = doc["bench"]
        L += ["", "## The flagship benchmark, same box, same call", "",
              "`%s`: %s with this library, %s with the parent's (the MSM path is not touched)." % (b["command"], b["this"], b["parent"])]
    if doc.get("notes"):
        L += ["", "## Notes", ""] + doc["notes"]
    with open(os.path.splitext(OUT)[0] + ".md", "w") as f:
        f.write("\n".join(L) + "\n")


def take_resources(path):
    kernels, cur = [], None
    for ln in open(path):
        m = re.search(r"remark: +(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        key, val = m.groups()
        if key == "Function Name":
            name = next((kn for kn in KERNELS if kn in val), None)
            cur = None
            if name:
                wire = "ILb1E" in val
                cur = {"kernel": name + ("<wire>" if wire else "<device format>" if name == "k_g1_decode_be" else "")}
                kernels.append(cur)
        elif cur is not None:
            cur[{"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
                 "LDS Size [bytes/block]": "lds"}[key]] = int(val)
    return kernels


def take_kernel_stats(path, what):
    rows = []
    for rec in csv.DictReader(open(path)):
        name = rec.get("Name", "")
        kn = next((kn for kn in KERNELS if kn in name), None)
        if kn:
            wire = "<true>" in name or "ILb1E" in name
            label = kn + (("<wire>" if wire else "<device format>") if kn == "k_g1_decode_be" else "")
            rows.append({"kernel": label, "calls": int(rec["Calls"]), "total_us": float(rec["TotalDurationNs"]) / 1e3, "avg_us": float(rec["AverageNs"]) / 1e3,
                         "min_us": float(rec["MinNs"]) / 1e3, "max_us": float(rec["MaxNs"]) / 1e3})
    return {"what": what, "rows": rows}


if len(sys.argv) > 1 and sys.argv[1] != "--trace-child":
    doc = load_json()
    if sys.argv[1] == "--resources":
        doc["kernels"] = take_resources(sys.argv[2])
    elif sys.argv[1] == "--kernel-stats":
        doc["kernel_trace"] = take_kernel_stats(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "")
    elif sys.argv[1] == "--bench":
        p, t = (json.loads(open(x).read().strip().splitlines()[-1]) for x in sys.argv[2:4])
        line = lambda j: "%.4f ms per step (%.4g %s)" % (j.get("ms_per_step", float("nan")), j.get("value", float("nan")), j.get("unit", ""))   # noqa: E731
        keep = lambda j: {kk: j.get(kk) for kk in ("value", "unit", "ms_per_step", "steps", "warmup", "n_gpus")}                                      # noqa: E731
        doc["bench"] = {"command": "python bench.py --gpus 1 --steps 20 --warmup 5", "parent": line(p), "this": line(t), "parent_line": keep(p), "this_line": keep(t)}
    elif sys.argv[1] != "--render":
        sys.exit(__doc__)
    save_json(doc)
    render(doc)
    sys.exit(0)

import numpy as np
import bench
import rust_kzg_bn254_amd as k
from rust_kzg_bn254_amd import _lib

LOG_N = 16
N_DOMAIN = 1 << LOG_N
REPS = int(os.environ.get("CB_REPS", "7"))
D_REPS = int(os.environ.get("CB_D_REPS", "3"))
ROWS = [(65536, 64), (65536, 16), (65536, 1), (4096, 16), (256, 16)]
if os.environ.get("CB_ROWS"):
    ROWS = [tuple(int(v) for v in r.split(",")) for r in os.environ["CB_ROWS"].split(";")]
VARIANTS = [v for v in "abcd" if v in os.environ.get("CB_VARIANTS", "a,b,c,d").split(",")]
TRACE_CHILD = "--trace-child" in sys.argv
tau = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % bench.FR
ctx = k.Context(0)
srs = k.SRS.generate(tau, N_DOMAIN, ctx=ctx)
kz = k.KZG.new(ctx)
kz.calculate_and_store_roots_of_unity(N_DOMAIN * 32)
u64p, u8p, vp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.c_void_p
P = _lib.ptr

parent = None
if "a" in VARIANTS or "d" in VARIANTS:
    path = os.environ.get("CB_BASELINE_LIB")
    assert path and os.path.exists(path), "CB_BASELINE_LIB must name the parent commit's library"
    plib = C.CDLL(path)
    plib.kzg_ctx_create.argtypes = [C.c_int32, C.POINTER(vp)]
    plib.kzg_srs_generate.argtypes = [vp, u64p, C.c_uint64, C.c_size_t, C.POINTER(vp)]
    plib.kzg_verify_multiproof_batch.argtypes = [vp, vp, u64p, C.c_size_t, u64p, u64p, u64p, u64p, C.c_size_t, C.c_size_t, C.c_size_t, u64p, u64p, C.POINTER(C.c_int32)]
    plib.kzg_srs_load_compressed_be.argtypes = [vp, u8p, C.c_size_t, C.POINTER(vp), u64p]
    plib.kzg_srs_download.argtypes = [vp, vp, C.c_size_t, C.c_size_t, u64p]
    plib.kzg_srs_free.argtypes = [vp]
    plib.kzg_srs_free.restype = None
    pctx, psrs = vp(), vp()
    assert plib.kzg_ctx_create(0, C.byref(pctx)) == 0
    assert plib.kzg_srs_generate(pctx, P(k.fr.fr_from_int(tau)), 0, N_DOMAIN, C.byref(psrs)) == 0
    parent = (plib, pctx, psrs)


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
    cm, ys, pf = np.ascontiguousarray(np.stack(commitments)), np.ascontiguousarray(np.concatenate(ys)), np.ascontiguousarray(np.concatenate(proofs))
    ys_be, pf_be = k.verifier.encode_coset_items(ys, pf)
    f = lambda b: np.frombuffer(b, np.uint8)                                                        # noqa: E731
    return {"cm": cm, "ci": np.array(rows, np.uint64), "ki": np.array(ks, np.uint64), "ys": ys, "pf": pf, "g2": g2, "cm_be": f(k.helpers.compress_g1_be(cm)),
            "ys_be": f(ys_be), "pf_be": f(pf_be)}


def verify_parent(cm, it, ys, pf, N, l):
    ok = C.c_int32(0)
    rc = parent[0].kzg_verify_multiproof_batch(parent[1], parent[2], P(cm), len(cm), P(it["ci"]), P(it["ki"]), P(ys), P(pf), N, N_DOMAIN, l, None, P(it["g2"]), C.byref(ok))
    assert rc == 0 and ok.value == 1, ("parent", rc, ok.value)


def points_through_the_srs_loader(buf):
    plib, n = parent[0], len(buf) // 32
    h, bad, out = vp(), C.c_uint64(0), np.zeros((n, 8), np.uint64)
    assert plib.kzg_srs_load_compressed_be(parent[1], buf.ctypes.data_as(u8p), n, C.byref(h), C.byref(bad)) == 0
    assert plib.kzg_srs_download(parent[1], h, 0, n, P(out)) == 0
    plib.kzg_srs_free(h)
    return out


def call(v, it, N, l):
    lib, h = _lib.load(), ctx.handle
    B = lambda a: a.ctypes.data_as(u8p)                                                              # noqa: E731
    if v == "a":
        verify_parent(it["cm"], it, it["ys"], it["pf"], N, l)
    elif v == "b":
        ys, pf, cm = np.empty((N, l, 4), np.uint64), np.empty((N, 8), np.uint64), np.empty((len(it["cm"]), 8), np.uint64)
        assert lib.kzg_coset_items_decode_be(h, B(it["ys_be"]), B(it["pf_be"]), N, l, P(ys), P(pf), None, None) == 0
        assert lib.kzg_g1_decompress_be_device(h, B(it["cm_be"]), len(cm), P(cm), None, None) == 0
    elif v == "c":
        ok = C.c_int32(0)
        rc = lib.kzg_verify_multiproof_batch_bytes(h, srs.handle, B(it["cm_be"]), len(it["cm"]), P(it["ci"]), P(it["ki"]), B(it["ys_be"]), B(it["pf_be"]), N, N_DOMAIN, l,
                                                   None, P(it["g2"]), C.byref(ok), None, None, None)
        assert rc == 0 and ok.value == 1, ("bytes", rc, ok.value)
    else:
        os.environ["KZG_NO_PRECOMPUTE"] = "1"
        try:
            pf, cm = points_through_the_srs_loader(it["pf_be"]), points_through_the_srs_loader(it["cm_be"])
        finally:
            del os.environ["KZG_NO_PRECOMPUTE"]
        raw = it["ys_be"].tobytes()
        ys = k.fr.frs_from_ints([int.from_bytes(raw[i:i + 32], "big") for i in range(0, len(raw), 32)]).reshape(N, l, 4)
        verify_parent(cm, it, ys, pf, N, l)


results = []
for N, l in ROWS:
    it = build_items(N, l)
    if TRACE_CHILD:
        for v in [v for v in VARIANTS if v in "ac"]:
            print("VARIANT %s" % v, file=sys.stderr, flush=True)
            for _ in range(6):                                                                   # the first is the warm-up the parent process drops
                call(v, it, N, l)
        continue
    d_reps = REPS if N * l <= 1 << 16 else min(REPS, D_REPS)
    for v in VARIANTS:
        if v != "d" or N * l <= 1 << 16:                                                         # (the slow codec is its own warm-up: nothing of it is cached)
            call(v, it, N, l)
    times = {v: [] for v in VARIANTS}
    for rep in range(REPS):
        for v in VARIANTS:
            if v == "d" and rep >= d_reps:
                continue
            t0 = time.perf_counter()
            call(v, it, N, l)
            times[v].append((time.perf_counter() - t0) * 1e3)
    row = {"N": N, "chunk_len": l, "n": N_DOMAIN, "commitments": len(it["cm"]), "values_bytes": N * l * 32, "rounds": REPS, "d_rounds": d_reps}
    for v in VARIANTS:
        row[v + "_ms"] = {"median": round(statistics.median(times[v]), 3), "min": round(min(times[v]), 3), "max": round(max(times[v]), 3)}
    if (N, l) in GATE_ROWS and all(v in VARIANTS for v in "abc"):
        row["gate_bound_ms"] = round((row["a_ms"]["median"] + row["b_ms"]["median"]) * 1.05, 3)
        row["gate_met"] = row["c_ms"]["median"] <= row["gate_bound_ms"]
    results.append(row)
    print(json.dumps(row), flush=True)

if TRACE_CHILD:
    sys.exit(0)
if not os.environ.get("CB_NO_TRACE") and any(v in VARIANTS for v in "ac"):
    env = dict(os.environ, KZG_VB_TRACE="1", CB_ROWS=";".join("%d,%d" % r for r in ROWS), CB_VARIANTS=",".join(v for v in VARIANTS if v in "ac"))
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child"], env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    seen, variant = {}, None
    for ln in res.stderr.splitlines():
        if ln.startswith("VARIANT "):
            variant = ln.split()[1]
        mt = re.match(r"kzg_verify_multiproof_batch(?:_bytes)? N=(\d+) l=(\d+) M=\d+: (.*)", ln)
        if mt:
            text = re.sub(r"\([^()]*\)", "", mt.group(3))                                        # (the parenthesised remarks carry figures of their own)
            phases = [(name.strip(" ,"), float(ms)) for name, ms in re.findall(r"([A-Za-z_+/ ]+?) ([0-9.]+) ms", text)]
            seen.setdefault((int(mt.group(1)), int(mt.group(2)), variant), []).append(phases)
    for row in results:
        for v in "ac":
            calls = seen.get((row["N"], row["chunk_len"], v), [])[1:]
            if calls:
                row[v + "_traced_phase_ms"] = {name: round(statistics.median(c[i][1] for c in calls), 3) for i, (name, _) in enumerate(calls[0])}
        print(json.dumps({kk: vv for kk, vv in row.items() if "traced" in kk or kk in ("N", "chunk_len")}), flush=True)

doc = load_json()
doc["rows"] = results
save_json(doc)
render(doc)
