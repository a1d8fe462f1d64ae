"""Per-call time of the disperser's serialized-form entries next to the route a caller had before them, from host buffers to host buffers
(every timed window ends in the call's own device synchronisation), same process, same device, variants taken in turns inside each round:

  E   this library: kzg_encode_cosets_batch_bytes (commitments, values, proofs)
  e   the route before it, on the PARENT commit's library (EBY_BASELINE_LIB, loaded beside this one, its own context and SRS):
      kzg_encode_cosets_batch, kzg_commit_coeff_form_batch, kzg_coset_items_encode_be (the C host encoder: the cheapest codec a caller has).
      The host decode of the blob (big-endian bytes -> Montgomery words) that the route starts with is done ONCE outside the window: the
      library has no host-only decoder to charge it with
  D   this library: kzg_disperse_blobs_bytes (headers and chunks)
  d   e plus kzg_commit_with_length_proof_batch and kzg_header_items_encode_be on the parent's library (its commitments stand for those of
      kzg_commit_coeff_form_batch, which d then leaves out)

The route is therefore UNDER-charged: its blob decode is free.  Shapes as profiles/encode_batch.md: (d = 2^12, r = 8, l = 16) at B = 1, 16, 64;
(2^14, 8, 16), (2^16, 8, 16) and (2^14, 8, 1) at B = 16.  At most EBY_DISTINCT = 2 distinct blobs, repeated to B (the calls do the same work on
repeated data).  Before anything is timed E must equal e and D must equal d byte for byte.  One warm-up per variant, then EBY_REPS (7) rounds:
median, min, max in ms per call.  The rule: median(E) <= median(e) and median(D) <= median(d) at B >= 16, median <= the route's max at B = 1.
EBY_SHAPES="log_d:log_r:l:B,..." overrides the shapes; EBY_RESOURCES names the outputs (comma separated) of
`hipcc -Rpass-analysis=kernel-resource-usage -c` on multiproof.hip and g1fft.hip whose figures go into the table; EBY_BENCH_LINES names a file of
bench.py result lines (label<TAB>json) recorded in the same session; writes EBY_OUT (profiles/encode_bytes.json) and renders
profiles/encode_bytes.md beside it (--render: render only)."""
import ctypes as C, hashlib, json, os, re, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.environ.get("EBY_OUT", os.path.join(ROOT, "profiles", "encode_bytes.json"))
KERNELS = {"k_encode_gather_cosetsILb0E": "k_encode_gather_cosets<words>", "k_encode_gather_cosetsILb1E": "k_encode_gather_cosets<bytes>",
           "k_encode_place_coeffsILb0E": "k_encode_place_coeffs<words>", "k_encode_place_coeffsILb1E": "k_encode_place_coeffs<bytes>",
           "k_encode_decode_be": "k_encode_decode_be", "k_g1fft_to_affineILb0E": "k_g1fft_to_affine<words>", "k_g1fft_to_affineILb1E": "k_g1fft_to_affine<bytes>",
           "k_g1fft_to_affineEPKijP": "k_g1fft_to_affine (parent)", "k_encode_gather_cosetsEPK": "k_encode_gather_cosets (parent)",
           "k_encode_place_coeffsEPK": "k_encode_place_coeffs (parent)"}


def fmt(c):
    return "–" if not c else "%.3f [%.3f, %.3f]" % (c["median"], c["min"], c["max"])


def render(doc):
    L = ["# Blobs encoded from bytes to serialized chunks and headers (`kzg_encode_cosets_batch_bytes`, `kzg_disperse_blobs_bytes`): measured on one MI355X", "",
         "`python tools/time_encode_bytes.py` (raw figures: `encode_bytes.json`).  Host buffers in, host buffers out, coefficient form;",
         "one warm-up per variant, then %d rounds with the variants taken in turns; **ms per call: median [min, max]**." % doc.get("reps", 0), "",
         "- **E** this library, `kzg_encode_cosets_batch_bytes` (commitments, values, proofs)",
         "- **e** the route before it: `kzg_encode_cosets_batch`, `kzg_commit_coeff_form_batch`, `kzg_coset_items_encode_be`",
         "- **D** this library, `kzg_disperse_blobs_bytes`",
         "- **d** `kzg_encode_cosets_batch`, `kzg_commit_with_length_proof_batch`, `kzg_coset_items_encode_be`, `kzg_header_items_encode_be`", "",
         "e and d consist only of entries this change does not touch; they ran on a build of the PARENT commit, loaded into the same process",
         "beside this library (its own context and SRS), in the same session on the same device.  The route's decode of the blob bytes to",
         "Montgomery words is NOT in its window (the library has no host-only decoder to charge it with): e and d are under-charged by that pass.",
         "Before timing, E equalled e and D equalled d byte for byte at every row.", "",
         "| d | r | l | B | bytes out | E | e | E / e | D | d | D / d | within the rule |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc.get("rows", []):
        ratio = lambda a, b: "%.2f" % (r[a]["median"] / r[b]["median"]) if r.get(a) and r.get(b) else "–"       # noqa: E731
        bound = "max" if r["blobs"] == 1 else "median"
        verdict = ", ".join("%s %s" % (a, "yes" if r[a]["median"] <= r[b][bound] else "NO") for a, b in (("E", "e"), ("D", "d")) if r.get(a) and r.get(b))
        L.append("| 2^%d | %d | %d | %d | %.2f MiB | %s | %s | %s | %s | %s | %s | %s (≤ the route's %s) |" % (
            r["log_d"], 1 << r["log_r"], r["chunk_len"], r["blobs"], r["bytes_out"] / 2 ** 20, fmt(r.get("E")), fmt(r.get("e")), ratio("E", "e"), fmt(r.get("D")),
            fmt(r.get("d")), ratio("D", "d"), verdict, bound))
    if doc.get("host_pass"):
        L += ["", "## The host pass the route ends in (`kzg_coset_items_encode_be` on the downloaded words), alone", "",
              "| d | r | l | B | ms: median [min, max] | share of e |", "|---|---|---|---|---|---|"]
        for h in doc["host_pass"]:
            L.append("| 2^%d | %d | %d | %d | %s | %.0f %% |" % (h["log_d"], 1 << h["log_r"], h["chunk_len"], h["blobs"], fmt(h["t"]), 100 * h["share"]))
    if doc.get("bench"):
        L += ["", "## The flagship line (`python bench.py --gpus 1`, 50 steps), same session, in this order", "", "| build | ms per step | pairs / s |", "|---|---|---|"]
        for b in doc["bench"]:
            line = json.loads(b["line"])
            L.append("| %s | %.4f | %.4g |" % (b["label"], line["ms_per_step"], line["value"]))
    if doc.get("kernels"):
        L += ["", "## The kernels (compiler figures, `-Rpass-analysis=kernel-resource-usage`, gfx950, cross-compiled)", "",
              "| kernel | VGPRs | SGPRs | LDS bytes / workgroup | waves / SIMD | scratch |", "|---|---|---|---|---|---|"]
        for kk in doc["kernels"]:
            L.append("| `%s` | %d | %d | %d | %d | %d |" % (kk["kernel"], kk["vgprs"], kk["sgprs"], kk["lds"], kk["occupancy"], kk["scratch"]))
    if doc.get("notes"):
        L += [""] + doc["notes"]
    with open(os.path.splitext(OUT)[0] + ".md", "w") as f:
        f.write("\n".join(L) + "\n")


def take_resources(paths):
    kernels = []
    for path in paths.split(","):
        cur = None
        for ln in open(path):
            m = re.search(r"remark: +(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
            if not m:
                continue
            key, val = m.groups()
            if key == "Function Name":
                name = next((v for kk, v in KERNELS.items() if kk in val), None)
                cur = {"kernel": name} if name else None
                if cur and not any(o["kernel"] == name for o in kernels):
                    kernels.append(cur)
            elif cur is not None:
                cur[{"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
                     "LDS Size [bytes/block]": "lds"}[key]] = int(val)
    return sorted(kernels, key=lambda kk: kk["kernel"])


doc = json.load(open(OUT)) if os.path.exists(OUT) else {}
if os.environ.get("EBY_RESOURCES"):
    doc["kernels"] = take_resources(os.environ["EBY_RESOURCES"])
if os.environ.get("EBY_BENCH_LINES"):
    doc["bench"] = [{"label": ln.split("\t", 1)[0], "line": ln.split("\t", 1)[1].strip()} for ln in open(os.environ["EBY_BENCH_LINES"]) if "\t" in ln]
if os.environ.get("EBY_NOTES"):
    doc["notes"] = [ln.rstrip("\n") for ln in open(os.environ["EBY_NOTES"])]
if "--render" in sys.argv:
    json.dump(doc, open(OUT, "w"), indent=1)
    render(doc)
    sys.exit(0)

import numpy as np
import torch  # noqa: F401  (load order: see tests/conftest.py)
import bench
import rust_kzg_bn254_amd as k
from rust_kzg_bn254_amd import _lib

lib = _lib.load()
P = _lib.ptr
u64p, u8p, vp, sz = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.c_void_p, C.c_size_t
B8 = lambda a: a.ctypes.data_as(u8p)                                                                # noqa: E731
REPS = int(os.environ.get("EBY_REPS", "7"))
DISTINCT = int(os.environ.get("EBY_DISTINCT", "2"))
shapes = [[int(v) for v in s.split(":")] for s in os.environ.get("EBY_SHAPES", "12:3:16:1,12:3:16:16,12:3:16:64,14:3:16:16,16:3:16:16,14:3:1:16").split(",")]
tau = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % bench.FR
max_d = max(1 << s[0] for s in shapes)
ORDER = 1 << 28
ctx = k.Context(0)
srs = k.SRS.generate(tau, max_d, ctx=ctx)
g2 = k.G2SRS.generate(tau, max_d, ctx=ctx)
trailing = k.G2SRS.generate(tau, max_d, first_power=ORDER - max_d, ctx=ctx)

path = os.environ.get("EBY_BASELINE_LIB")
assert path and os.path.exists(path), "EBY_BASELINE_LIB must name the parent commit's library"
plib = C.CDLL(path)
plib.kzg_ctx_create.argtypes = [C.c_int32, C.POINTER(vp)]
plib.kzg_srs_generate.argtypes = [vp, u64p, C.c_uint64, sz, C.POINTER(vp)]
plib.kzg_g2srs_generate.argtypes = [vp, u64p, C.c_uint64, sz, C.POINTER(vp)]
plib.kzg_encode_cosets_batch.argtypes = [vp, vp, u64p, sz, sz, C.c_int32, sz, sz, u64p, u64p, u8p]
plib.kzg_commit_coeff_form_batch.argtypes = [vp, vp, u64p, sz, sz, u64p, u8p]
plib.kzg_commit_with_length_proof_batch.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_uint64, u64p, sz, sz, C.c_uint64, u64p, u64p, u64p]
plib.kzg_coset_items_encode_be.argtypes = [u64p, u64p, sz, sz, u8p, u8p]
plib.kzg_header_items_encode_be.argtypes = [u64p, u64p, u64p, sz, u8p, u8p, u8p]
pctx, psrs, pg2, ptr_ = vp(), vp(), vp(), vp()
tau_w = k.fr.fr_from_int(tau)
assert plib.kzg_ctx_create(0, C.byref(pctx)) == 0
assert plib.kzg_srs_generate(pctx, P(tau_w), 0, max_d, C.byref(psrs)) == 0
assert plib.kzg_g2srs_generate(pctx, P(tau_w), 0, max_d, C.byref(pg2)) == 0
assert plib.kzg_g2srs_generate(pctx, P(tau_w), ORDER - max_d, max_d, C.byref(ptr_)) == 0

rows, host_pass = [], []
for log_d, log_r, l, B in shapes:
    d, n = 1 << log_d, 1 << (log_d + log_r)
    m = n // l
    distinct = min(DISTINCT, B)
    ints = [bench.uniform_scalars(d, 11 * log_d + b)[0] for b in range(distinct)]
    blob1 = [b"".join(int(v).to_bytes(32, "big") for v in row) for row in ints]
    blobs = np.frombuffer(b"".join(blob1[b % distinct] for b in range(B)), np.uint8)
    words = np.ascontiguousarray(np.stack([bench.ints_to_wire(ints[b % distinct]) for b in range(B)]))     # the route's decode, outside its window
    cmE, ysE, pfE, cme, yse, pfe = (np.zeros(B * s, np.uint8) for s in (32, n * 32, m * 32) * 2)
    cmD, c2D, p2D, ysD, pfD = (np.zeros(B * s, np.uint8) for s in (32, 64, 64, n * 32, m * 32))
    cmd, c2d, p2d = (np.zeros(B * s, np.uint8) for s in (32, 64, 64))
    ys_w, pf_w, inf_w = np.zeros((B * n, 4), np.uint64), np.zeros((B * m, 8), np.uint64), np.zeros(B * m, np.uint8)
    cm_w, c2_w, p2_w = np.zeros((B, 8), np.uint64), np.zeros((B, 16), np.uint64), np.zeros((B, 16), np.uint64)

    def E():
        assert lib.kzg_encode_cosets_batch_bytes(ctx.handle, srs.handle, B8(blobs), B, d, 0, n, l, B8(cmE), B8(ysE), B8(pfE), None) == 0

    def chunks_route():
        assert plib.kzg_encode_cosets_batch(pctx, psrs, P(words), B, d, 0, n, l, P(ys_w), P(pf_w), B8(inf_w)) == 0

    def host_encode():
        assert plib.kzg_coset_items_encode_be(P(ys_w), P(pf_w), B * m, l, B8(yse), B8(pfe)) == 0

    def e():
        chunks_route()
        assert plib.kzg_commit_coeff_form_batch(pctx, psrs, P(words), d, B, P(cm_w), None) == 0
        host_encode()
        assert plib.kzg_coset_items_encode_be(None, P(cm_w), B, 1, None, B8(cme)) == 0

    def D():
        assert lib.kzg_disperse_blobs_bytes(ctx.handle, srs.handle, g2.handle, trailing.handle, ORDER - max_d, ORDER, B8(blobs), B, d, n, l, d, B8(cmD), B8(c2D), B8(p2D),
                                            B8(ysD), B8(pfD), None) == 0

    def dd():
        chunks_route()
        assert plib.kzg_commit_with_length_proof_batch(pctx, psrs, pg2, ptr_, ORDER - max_d, ORDER, P(words), d, B, d, P(cm_w), P(c2_w), P(p2_w)) == 0
        host_encode()
        assert plib.kzg_header_items_encode_be(P(cm_w), P(c2_w), P(p2_w), B, B8(cmd), B8(c2d), B8(p2d)) == 0

    variants = {"E": E, "e": e, "D": D, "d": dd}
    for fn in variants.values():                                                               # the warm-up, and the outputs to compare
        fn()
    assert np.array_equal(cmE, cme) and np.array_equal(ysE, yse) and np.array_equal(pfE, pfe), "E differs from its route"
    assert all(np.array_equal(a, b) for a, b in ((cmD, cmd), (c2D, c2d), (p2D, p2d), (ysD, yse), (pfD, pfe))), "D differs from its route"
    times = {name: [] for name in list(variants) + ["host"]}
    for _ in range(REPS):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        host_encode()
        times["host"].append((time.perf_counter() - t0) * 1e3)
    stat = lambda ts: {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}   # noqa: E731
    row = {"log_d": log_d, "log_r": log_r, "chunk_len": l, "blobs": B, "bytes_out": B * (32 + n * 32 + m * 32), "distinct_blobs": distinct}
    for name in variants:
        row[name] = stat(times[name])
    rows.append(row)
    host_pass.append({"log_d": log_d, "log_r": log_r, "chunk_len": l, "blobs": B, "t": stat(times["host"]),
                      "share": round(statistics.median(times["host"]) / statistics.median(times["e"]), 3)})
    print(json.dumps(row), flush=True)

doc["rows"], doc["host_pass"], doc["reps"] = rows, host_pass, REPS
json.dump(doc, open(OUT, "w"), indent=1)
render(doc)
