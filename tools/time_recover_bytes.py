"""Per-call time of the retriever's serialized-form entries next to the routes a caller had before them, from host buffers to host buffers
(every timed window ends in the call's own device synchronisation), same process, same device, variants taken in turns inside each round:

  R   this library: kzg_recover_from_cosets_batch_bytes
  r   the route before it, on the PARENT commit's library (RBY_BASELINE_LIB, loaded beside this one, its own context): kzg_coset_items_decode_be,
      kzg_recover_from_cosets_batch, kzg_coset_items_encode_be (the C host encoder: the cheapest codec a caller has)
  V   this library: kzg_retrieve_blobs_bytes
  v   the parent's kzg_verify_multiproof_batch_bytes in front of r

Shapes as profiles/recover_batch.md: (2^13, l = 1) and (2^16, 64) with half of the cosets missing, (2^20, 16) with one coset missing, at
B in RBY_BLOBS (1, 16, 64; the largest shape up to 16).  The blobs are polynomials of n / 2 coefficients encoded by KZG.encode_cosets_batch
on a known-tau SRS (at most RBY_DISTINCT = 2 distinct blobs, repeated to B: the calls do the same work on repeated data), evaluation form
out, one index row for all blobs.  Before anything is timed R must equal r byte for byte and V must accept and equal R.  One warm-up per
variant, then RBY_REPS (7) rounds: median, min, max in ms per call.  The rule: R (V) is not slower than r (v) beyond r's (v's) own spread,
i.e. median(R) <= max(r).  RBY_SHAPES="log_n:l:missing:maxB,..." overrides the shapes (RBY_APPEND=1 keeps the file's other rows); RBY_RESOURCES names the output of
`hipcc -Rpass-analysis=kernel-resource-usage -c recover.hip` whose figures go into the table; writes RBY_OUT (profiles/recover_bytes.json) and
renders profiles/recover_bytes.md beside it (--render: render only)."""
import ctypes as C, hashlib, json, os, re, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.environ.get("RBY_OUT", os.path.join(ROOT, "profiles", "recover_bytes.json"))
KERNELS = {"k_recover_scatterILb0E": "k_recover_scatter<words>", "k_recover_scatterILb1E": "k_recover_scatter<bytes>", "k_recover_scaleILi2ELb0E": "k_recover_scale<2, words>",
           "k_recover_scaleILi2ELb1E": "k_recover_scale<2, bytes>", "k_fr_encode_be": "k_fr_encode_be"}


def fmt(c):
    return "–" if not c else "%.3f [%.3f, %.3f]" % (c["median"], c["min"], c["max"])


def render(doc):
    L = ["# Blobs recovered from serialized chunks (`kzg_recover_from_cosets_batch_bytes`, `kzg_retrieve_blobs_bytes`): measured on one MI355X", "",
         "`python tools/time_recover_bytes.py` (raw figures: `recover_bytes.json`).  Host buffers in, host buffers out, evaluation form, one index row;",
         "one warm-up per variant, then %d rounds with the variants taken in turns; **ms per call: median [min, max]**." % doc.get("reps", 0), "",
         "- **R** this library, `kzg_recover_from_cosets_batch_bytes`",
         "- **r** the route before it: `kzg_coset_items_decode_be`, `kzg_recover_from_cosets_batch`, `kzg_coset_items_encode_be`",
         "- **V** this library, `kzg_retrieve_blobs_bytes`",
         "- **v** `kzg_verify_multiproof_batch_bytes` in front of r", "",
         "r and v consist only of entries this change does not touch; they ran on a build of the PARENT commit, loaded into the same process",
         "beside this library (its own context and SRS), in the same session on the same device.  Before timing, R equalled r byte for byte and V",
         "accepted and equalled R at every row.", "",
         "| n | l | missing | B | value bytes in | R | r | R / r | V | v | V / v | not slower (median ≤ the route's max) |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc.get("rows", []):
        ratio = lambda a, b: "%.2f" % (r[a]["median"] / r[b]["median"]) if r.get(a) and r.get(b) else "–"       # noqa: E731
        verdict = ", ".join("%s %s" % (a, "yes" if r[a]["median"] <= r[b]["max"] else "NO") for a, b in (("R", "r"), ("V", "v")) if r.get(a) and r.get(b))
        L.append("| 2^%d | %d | %d | %d | %.1f MiB | %s | %s | %s | %s | %s | %s | %s |" % (r["log_n"], r["chunk_len"], r["missing"], r["blobs"], r["value_bytes"] / 2 ** 20,
                                                                                       fmt(r.get("R")), fmt(r.get("r")), ratio("R", "r"), fmt(r.get("V")), fmt(r.get("v")),
                                                                                       ratio("V", "v"), verdict))
    if doc.get("kernels"):
        L += ["", "## The kernels (compiler figures, `-Rpass-analysis=kernel-resource-usage`, gfx950, cross-compiled)", "",
              "| kernel | VGPRs | SGPRs | LDS bytes / workgroup | waves / SIMD | scratch |", "|---|---|---|---|---|---|"]
        for kk in doc["kernels"]:
            L.append("| `%s` | %d | %d | %d | %d | %d |" % (kk["kernel"], kk["vgprs"], kk["sgprs"], kk["lds"], kk["occupancy"], kk["scratch"]))
    if doc.get("notes"):
        L += [""] + doc["notes"]
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
            name = next((v for kk, v in KERNELS.items() if kk in val), None)
            cur = {"kernel": name} if name else None
            if cur:
                kernels.append(cur)
        elif cur is not None:
            cur[{"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
                 "LDS Size [bytes/block]": "lds"}[key]] = int(val)
    return sorted(kernels, key=lambda kk: kk["kernel"])


doc = json.load(open(OUT)) if os.path.exists(OUT) else {}
if os.environ.get("RBY_RESOURCES"):
    doc["kernels"] = take_resources(os.environ["RBY_RESOURCES"])
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
u64p, u8p, vp, sz, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)
B8 = lambda a: a.ctypes.data_as(u8p)                                                                # noqa: E731
REPS = int(os.environ.get("RBY_REPS", "7"))
DISTINCT = int(os.environ.get("RBY_DISTINCT", "2"))
shapes = [s.split(":") for s in os.environ.get("RBY_SHAPES", "13:1:half:64,16:64:half:64,20:16:one:16").split(",")]
batch_sizes = [int(b) for b in os.environ.get("RBY_BLOBS", "1,16,64").split(",")]
tau = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % bench.FR
max_d = max(1 << (int(s[0]) - 1) for s in shapes)
ctx = k.Context(0)
srs = k.SRS.generate(tau, max_d, ctx=ctx)
kz = k.KZG.new(ctx)

path = os.environ.get("RBY_BASELINE_LIB")
assert path and os.path.exists(path), "RBY_BASELINE_LIB must name the parent commit's library"
plib = C.CDLL(path)
plib.kzg_ctx_create.argtypes = [C.c_int32, C.POINTER(vp)]
plib.kzg_srs_generate.argtypes = [vp, u64p, C.c_uint64, sz, C.POINTER(vp)]
plib.kzg_coset_items_decode_be.argtypes = [vp, u8p, u8p, sz, sz, u64p, u64p, u64p, i32p]
plib.kzg_recover_from_cosets_batch.argtypes = [vp, u64p, u64p, sz, sz, sz, sz, sz, sz, C.c_int32, sz, u64p, i32p]
plib.kzg_coset_items_encode_be.argtypes = [u64p, u64p, sz, sz, u8p, u8p]
plib.kzg_verify_multiproof_batch_bytes.argtypes = [vp, vp, u8p, sz, u64p, u64p, u8p, u8p, sz, sz, sz, u64p, u64p, i32p, u64p, u64p, i32p]
pctx, psrs = vp(), vp()
assert plib.kzg_ctx_create(0, C.byref(pctx)) == 0
assert plib.kzg_srs_generate(pctx, P(k.fr.fr_from_int(tau)), 0, 4096, C.byref(psrs)) == 0      # the verifier reads l <= 64 of its points

rows = []
for log_n, l, missing, max_b in shapes:
    log_n, l, max_b = int(log_n), int(l), int(max_b)
    n = 1 << log_n
    m, d = n // l, n // 2
    idx = np.arange(0, m, 2, dtype=np.uint64) if missing == "half" else np.arange(0, m - 1, dtype=np.uint64)
    count = len(idx)
    distinct = min(DISTINCT, max(b for b in batch_sizes if b <= max_b))
    coeffs = np.stack([bench.ints_to_wire(bench.uniform_scalars(d, 7 * log_n + b)[0]) for b in range(distinct)])
    polys = [k.PolynomialCoeffForm(c) for c in coeffs]
    ys_all, pf_all = kz.encode_cosets_batch(polys, srs, n, l)
    cm = np.stack([kz.commit_coeff_form(p, srs) for p in polys])
    g2 = k.helpers.g2_mul_generator(k.fr.fr_from_int(pow(tau, l, bench.FR)))
    pick = idx.astype(np.int64)
    ys1, pf1 = k.verifier.encode_coset_items(np.ascontiguousarray(ys_all[:, pick]).reshape(-1, l, 4), np.ascontiguousarray(pf_all[:, pick]).reshape(-1, 8))
    cm1 = k.helpers.compress_g1_be(cm)
    del ys_all, pf_all
    for B in [b for b in batch_sizes if b <= max_b]:
        reps_of = lambda raw, per: np.frombuffer(b"".join(raw[(b % distinct) * per:(b % distinct + 1) * per] for b in range(B)), np.uint8)   # noqa: E731
        ys_be, pf_be, cm_be = reps_of(ys1, count * l * 32), reps_of(pf1, count * 32), reps_of(cm1, 32)
        N = B * count
        ci, ki = np.repeat(np.arange(B, dtype=np.uint64), count), np.tile(idx, B)
        out_R, out_r, out_V = (np.zeros(B * n * 32, np.uint8) for _ in range(3))
        words_in, words_out = np.zeros((N, l, 4), np.uint64), np.zeros((B, n, 4), np.uint64)
        flags = np.zeros(B, np.int32)
        ok = C.c_int32(0)

        def R():
            assert lib.kzg_recover_from_cosets_batch_bytes(ctx.handle, B8(ys_be), P(idx), 1, B, count, n, l, 0, 1, 0, B8(out_R), flags.ctypes.data_as(i32p), None) == 0

        def r():
            assert plib.kzg_coset_items_decode_be(pctx, B8(ys_be), None, N, l, P(words_in), None, None, None) == 0
            assert plib.kzg_recover_from_cosets_batch(pctx, P(words_in), P(idx), 1, B, count, n, l, 0, 1, 0, P(words_out), flags.ctypes.data_as(i32p)) == 0
            assert plib.kzg_coset_items_encode_be(P(words_out), None, B * n, 1, B8(out_r), None) == 0

        def V():
            rc = lib.kzg_retrieve_blobs_bytes(ctx.handle, srs.handle, B8(cm_be), P(idx), 1, B8(ys_be), B8(pf_be), B, count, n, l, 0, 1, 0, None, P(g2), C.byref(ok), B8(out_V),
                                              flags.ctypes.data_as(i32p), None, None)
            assert rc == 0 and ok.value == 1, (rc, ok.value)

        def v():
            rc = plib.kzg_verify_multiproof_batch_bytes(pctx, psrs, B8(cm_be), B, P(ci), P(ki), B8(ys_be), B8(pf_be), N, n, l, None, P(g2), C.byref(ok), None, None, None)
            assert rc == 0 and ok.value == 1, (rc, ok.value)
            r()

        variants = {"R": R, "r": r, "V": V, "v": v}
        for fn in variants.values():                                                               # the warm-up, and the outputs to compare
            fn()
        assert np.array_equal(out_R, out_r) and np.array_equal(out_V, out_R) and flags.all(), "the routes differ"
        times = {name: [] for name in variants}
        for _ in range(REPS):
            for name, fn in variants.items():
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e3)
        row = {"log_n": log_n, "chunk_len": l, "missing": m - count, "blobs": B, "value_bytes": B * count * l * 32, "distinct_blobs": distinct}
        for name, ts in times.items():
            row[name] = {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)

if os.environ.get("RBY_APPEND"):                                                                 # keep the file's other rows (a shape measured in a run of its own)
    done = {(r["log_n"], r["chunk_len"], r["blobs"]) for r in rows}
    rows = sorted([r for r in doc.get("rows", []) if (r["log_n"], r["chunk_len"], r["blobs"]) not in done] + rows, key=lambda r: (r["log_n"], r["blobs"]))
doc["rows"], doc["reps"] = rows, REPS
json.dump(doc, open(OUT, "w"), indent=1)
render(doc)
