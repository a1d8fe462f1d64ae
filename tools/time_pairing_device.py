"""Pairing checks on the device, measured from host buffers to host buffers (every timed window ends in the call's own synchronisation), same
process, same device, the routes taken in turns inside each round.

(a) batches of two-pair checks e(P, Q) e(-P, Q) = 1:
  D   kzg_pairings_product_verify_batch, n checks in one call
  H   a loop of n calls of kzg_pairings_product_verify (host: two threaded Miller loops and one final exponentiation per call)
  n in PDT_CHECKS (1, 64, 1024, 4096).

(b) kzg_retrieve_blobs_bytes_tolerant on the rows of profiles/retrieve_tolerant.md (tools/time_retrieve_tolerant.py builds the same inputs):
  M0  this library, kzg_ctx_set_locate_pairings(ctx, 0): the host search
  M1  this library, mode 1: every group's equation on the device after a failing root
  p   the PARENT commit's library (PDT_BASELINE_LIB, built by tools/build_variant.sh, loaded beside this one, its own context and SRS), the same entry
  Shapes PDT_SHAPES="log_n:l:held:blobs,.." (16:64:513:64, 20:16:65535:16), cases PDT_CASES (none, one, three, eight, undecodable; at 2^20 the
  cases `three` and `eight` are left out unless PDT_ALL=1).  Before anything is timed the three routes must give the same statuses and rows.
  The rule, for the rows with nothing bad only: median(M1) <= max(p).

One warm-up per route, then PDT_REPS (7) rounds: median, min, max in ms per call.  PDT_RESOURCES names the output of `hipcc
-Rpass-analysis=kernel-resource-usage` over pairing.hip.  Writes PDT_OUT (profiles/pairing_device.json) and renders profiles/pairing_device.md
beside it (--render: render only; PDT_APPEND=1 keeps the file's other rows)."""
import ctypes as C, hashlib, json, os, re, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.environ.get("PDT_OUT", os.path.join(ROOT, "profiles", "pairing_device.json"))


def fmt(c):
    return "–" if not c else "%.3f [%.3f, %.3f]" % (c["median"], c["min"], c["max"])


def render(doc):
    L = ["# Pairing checks on the device (`kzg_pairings_product_verify_batch`, `kzg_ctx_set_locate_pairings`): measured on one MI355X", "",
         "`python tools/time_pairing_device.py` (raw figures: `pairing_device.json`).  Host buffers in, host buffers out; one warm-up per route, then %d rounds" % doc.get("reps", 0),
         "with the routes taken in turns; **ms per call: median [min, max]**.", "",
         "## (a) n two-pair checks: one device batch (D) against a loop of the host entry (H)", "",
         "| checks | D | H | H / D | D per check |", "|---|---|---|---|---|"]
    for r in doc.get("batch", []):
        L.append("| %d | %s | %s | %.2f | %.4f |" % (r["checks"], fmt(r["D"]), fmt(r["H"]), r["H"]["median"] / r["D"]["median"], r["D"]["median"] / r["checks"]))
    L += ["", "## (b) `kzg_retrieve_blobs_bytes_tolerant`: host search (M0), device leaves (M1), the parent commit's build (p)", "",
          "Before timing the three routes gave the same statuses and rows at every line.  The one rule is the project's own: with nothing bad,",
          "median(M1) ≤ max(p) -- mode 1 adds nothing to that path.  The other lines have no threshold; they are what was measured.", "",
          "| n | l | B | held | used | bad chunks | M0 | M1 | p | M1 / M0 | checks M0 | checks M1 | rule: median(M1) ≤ max(p) |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc.get("rows", []):
        rule = "–" if r["case"] != "none" else ("yes" if r["M1"]["median"] <= r["p"]["max"] else "**NO**")
        L.append("| 2^%d | %d | %d | %d | %d | %s | %s | %s | %s | %.2f | %d | %d | %s |" % (r["log_n"], r["chunk_len"], r["blobs"], r["held"], r["used"], r["case_text"], fmt(r["M0"]),
                                                                                     fmt(r["M1"]), fmt(r["p"]), r["M1"]["median"] / r["M0"]["median"], r["checks_M0"], r["checks_M1"], rule))
    if doc.get("kernels"):
        L += ["", "## The kernels (compiler figures, `-Rpass-analysis=kernel-resource-usage`, gfx950, cross-compiled)", "",
              "| kernel | VGPRs | AGPRs | SGPRs | scratch bytes / lane | LDS bytes / workgroup | waves / SIMD |", "|---|---|---|---|---|---|---|"]
        for kk in doc["kernels"]:
            L.append("| `%s` | %d | %d | %d | %d | %d | %d |" % (kk["kernel"], kk["vgprs"], kk["agprs"], kk["sgprs"], kk["scratch"], kk["lds"], kk["occupancy"]))
    if doc.get("notes"):
        L += [""] + doc["notes"]
    with open(os.path.splitext(OUT)[0] + ".md", "w") as f:
        f.write("\n".join(L) + "\n")


def take_resources(path):
    kernels, cur = [], None
    for ln in open(path):
        m = re.search(r"remark: +(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        key, val = m.groups()
        if key == "Function Name":
            name = next((v for v in ("k_pairing_convert", "k_pairing_checks") if v in val), None)
            cur = {"kernel": name} if name and not any(x["kernel"] == name for x in kernels) else None
            if cur:
                kernels.append(cur)
        elif cur is not None:
            cur[{"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
                 "LDS Size [bytes/block]": "lds"}[key]] = int(val)
    return kernels


doc = json.load(open(OUT)) if os.path.exists(OUT) else {}
if os.environ.get("PDT_RESOURCES"):
    doc["kernels"] = take_resources(os.environ["PDT_RESOURCES"])
if os.environ.get("PDT_NOTES"):
    doc["notes"] = [ln.rstrip("\n") for ln in open(os.environ["PDT_NOTES"])]
if "--render" in sys.argv:
    json.dump(doc, open(OUT, "w"), indent=1)
    render(doc)
    sys.exit(0)

import numpy as np
import torch  # noqa: F401  (load order: see tests/conftest.py)
import bench
import rust_kzg_bn254_amd as k
from rust_kzg_bn254_amd import _lib

sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyref

lib = _lib.load()
P = _lib.ptr
u64p, u8p, vp, sz, i32p, szp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_size_t)
B8 = lambda a: a.ctypes.data_as(u8p)                                                                # noqa: E731
REPS = int(os.environ.get("PDT_REPS", "7"))
CASES = os.environ.get("PDT_CASES", "none,one,three,eight,undecodable").split(",")
CHECKS = [int(v) for v in os.environ.get("PDT_CHECKS", "1,64,1024,4096").split(",") if v]
shapes = [[int(v) for v in s.split(":")] for s in os.environ.get("PDT_SHAPES", "16:64:513:64,20:16:65535:16").split(",") if s]
ctx = k.Context(0)


def stats(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def in_turns(routes):
    for fn in routes.values():
        fn()
    times = {name: [] for name in routes}
    for _ in range(REPS):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: stats(ts) for name, ts in times.items()}


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------------
batch = []
if CHECKS:
    g1 = [pyref.ec_mul(3 + 7 * i, (1, 2)) for i in range(16)]
    g2 = [k.helpers.g2_mul_generator(k.fr.fr_from_int(11 + 5 * i)) for i in range(8)]
    for n in CHECKS:
        a = np.stack([w for i in range(n) for w in (pyref.point_to_wire(g1[i % 16]), pyref.point_to_wire(pyref.ec_neg(g1[i % 16])))])
        b = np.stack([g2[(3 * i) % 8] for i in range(n) for _ in range(2)])
        off = np.arange(0, 2 * n + 1, 2, dtype=np.uint64)
        ok, one = np.zeros(n, np.uint8), C.c_int32(0)

        def D():
            assert lib.kzg_pairings_product_verify_batch(ctx.handle, P(a), P(b), P(off), n, B8(ok), None) == 0 and ok.all()

        def H():
            for i in range(n):
                assert lib.kzg_pairings_product_verify(P(a[2 * i:]), P(b[2 * i:]), 2, C.byref(one)) == 0 and one.value == 1

        row = {"checks": n}
        row.update(in_turns({"D": D, "H": H}))
        batch.append(row)
        print(json.dumps(row), flush=True)

# ---- (b) ------------------------------------------------------------------------------------------------------------------------------------
rows = []
if shapes:
    tau = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % bench.FR
    srs = k.SRS.generate(tau, max(1 << (s[0] - 1) for s in shapes), ctx=ctx)
    kz = k.KZG.new(ctx)
    path = os.environ.get("PDT_BASELINE_LIB")
    assert path and os.path.exists(path), "PDT_BASELINE_LIB must name the parent commit's library (tools/build_variant.sh)"
    plib = C.CDLL(path)
    plib.kzg_ctx_create.argtypes = [C.c_int32, C.POINTER(vp)]
    plib.kzg_srs_generate.argtypes = [vp, u64p, C.c_uint64, sz, C.POINTER(vp)]
    tol_args = [vp, vp, u8p, u64p, sz, u8p, u8p, sz, sz, sz, sz, sz, sz, C.c_int32, sz, u64p, u64p, u8p, u8p, szp, szp, szp, u8p, i32p, u64p, u64p, i32p]
    plib.kzg_retrieve_blobs_bytes_tolerant.argtypes = tol_args
    pctx, psrs = vp(), vp()
    assert plib.kzg_ctx_create(0, C.byref(pctx)) == 0
    assert plib.kzg_srs_generate(pctx, P(k.fr.fr_from_int(tau)), 0, 4096, C.byref(psrs)) == 0      # the verifier reads l <= 64 of its points
for log_n, l, held, B in shapes:
    n = 1 << log_n
    m, d = n // l, n // 2
    idx = np.array((list(range(0, m, 2)) + list(range(1, m, 2)))[:held], dtype=np.uint64)
    count = len(idx)
    distinct = min(2, B)
    coeffs = np.stack([bench.ints_to_wire(bench.uniform_scalars(d, 11 * log_n + b)[0]) for b in range(distinct)])
    polys = [k.PolynomialCoeffForm(c) for c in coeffs]
    ys_all, pf_all = kz.encode_cosets_batch(polys, srs, n, l)
    cm = np.stack([kz.commit_coeff_form(p, srs) for p in polys])
    g2 = k.helpers.g2_mul_generator(k.fr.fr_from_int(pow(tau, l, bench.FR)))
    pick = idx.astype(np.int64)
    ys1, pf1 = k.verifier.encode_coset_items(np.ascontiguousarray(ys_all[:, pick]).reshape(-1, l, 4), np.ascontiguousarray(pf_all[:, pick]).reshape(-1, 8))
    cm1 = k.helpers.compress_g1_be(cm)
    del ys_all, pf_all
    reps_of = lambda raw, per: np.frombuffer(b"".join(raw[(b % distinct) * per:(b % distinct + 1) * per] for b in range(B)), np.uint8).copy()   # noqa: E731
    ys_good, pf_good, cm_be = reps_of(ys1, count * l * 32), reps_of(pf1, count * 32), reps_of(cm1, 32)
    N = B * count
    for case, case_text, n_bad in (("none", "0", 0), ("one", "1 fails its equation", 1), ("three", "3 fail, in 3 blobs", 3), ("eight", "8 fail, in 8 blobs", 8), ("undecodable", "1 proof does not decode", 1)):
        if n_bad > B or case not in CASES or (case in ("three", "eight") and log_n >= 20 and not os.environ.get("PDT_ALL")):
            continue
        use = count if case == "none" else count - 1
        ys_be, pf_be = ys_good.copy(), pf_good.copy()
        for i in [(b * (B // max(n_bad, 1))) * count + (37 * (b + 1)) % count for b in range(n_bad)]:
            if case == "undecodable":
                pf_be[32 * i] &= 0x3F
            else:
                ys_be[32 * (i * l + 1) + 31] ^= 1
        outs = {r: (np.zeros(B * n * 32, np.uint8), np.zeros(B, np.int32), np.zeros(N, np.uint8), np.zeros(B, np.uint8), sz(0)) for r in ("M0", "M1", "p")}

        def call(which, entry, c, s, mode):
            out, flags, ist, bst, checks = outs[which]
            nb, nu = sz(0), sz(0)
            if mode is not None:
                ctx.set_locate_pairings(mode)
            rc = entry(c, s, B8(cm_be), P(idx), 1, B8(ys_be), B8(pf_be), B, count, use, n, l, 0, 1, 0, None, P(g2), B8(ist), B8(bst), C.byref(nb), C.byref(nu), C.byref(checks),
                       B8(out), flags.ctypes.data_as(i32p), None, None, None)
            assert rc == 0 and nu.value == 0 and nb.value == n_bad, (which, rc, nu.value, nb.value)

        routes = {"M0": lambda: call("M0", lib.kzg_retrieve_blobs_bytes_tolerant, ctx.handle, srs.handle, 0),
                  "M1": lambda: call("M1", lib.kzg_retrieve_blobs_bytes_tolerant, ctx.handle, srs.handle, 1),
                  "p": lambda: call("p", plib.kzg_retrieve_blobs_bytes_tolerant, pctx, psrs, None)}
        try:
            for fn in routes.values():
                fn()
            for r in ("M1", "p"):
                assert all(np.array_equal(x, y) for x, y in zip(outs["M0"][:4], outs[r][:4])), "the routes differ: " + r
            res = in_turns(routes)
        finally:
            ctx.set_locate_pairings(0)
        row = {"log_n": log_n, "chunk_len": l, "blobs": B, "held": count, "used": use, "case": case, "case_text": case_text, "checks_M0": int(outs["M0"][4].value),
               "checks_M1": int(outs["M1"][4].value)}
        row.update(res)
        rows.append(row)
        print(json.dumps(row), flush=True)

if os.environ.get("PDT_APPEND"):
    done = {(r["log_n"], r["chunk_len"], r["case"]) for r in rows}
    order = ["none", "one", "three", "eight", "undecodable"]
    rows = sorted([r for r in doc.get("rows", []) if (r["log_n"], r["chunk_len"], r["case"]) not in done] + rows, key=lambda r: (r["log_n"], order.index(r["case"])))
    batch = batch or doc.get("batch", [])
doc["rows"], doc["batch"], doc["reps"] = rows, batch, REPS
json.dump(doc, open(OUT, "w"), indent=1)
render(doc)
