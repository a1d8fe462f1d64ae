"""Per-call time of kzg_retrieve_blobs_bytes_tolerant next to what a caller does without it, from host buffers to host buffers (every timed
window ends in the call's own device synchronisation), same process, same device, the two routes taken in turns inside each round:

  T   this library: kzg_retrieve_blobs_bytes_tolerant
  t   the route before it, on the PARENT commit's library (RTT_BASELINE_LIB, built by tools/build_variant.sh, loaded beside this one, its own
      context and SRS): kzg_retrieve_blobs_bytes; if it rejects: kzg_coset_items_decode_be and kzg_g1_decompress_be_device,
      kzg_verify_multiproof_batch_locate by blob, the same by item over the items of the bad blobs, the good chunks reassembled on the host,
      kzg_recover_from_cosets_batch_bytes.  If a chunk does not decode, kzg_retrieve_blobs_bytes names it: the caller drops that chunk from
      every array (one index row per blob from then on) and calls again.

Rows: 64 blobs of 2^16 evaluations in chunks of 64 holding 513 of the 1024 cosets, 16 blobs of 2^20 in chunks of 16 holding all but one; each
with 0, 1 and 8 bad chunks (a flipped value byte) in distinct blobs and with one chunk whose proof does not decode.  With nothing bad every held
chunk is used (use_count = count: the row of the rule); the other rows use one chunk less than is held.  The blobs are polynomials of n / 2
coefficients on a known-tau SRS (RTT_DISTINCT = 2 distinct blobs repeated: the calls do the same work on repeated data).  Before anything is
timed T and t must give the same rows.  One warm-up per route, then RTT_REPS (7) rounds: median, min, max in ms per call.  The rule, for the
rows with nothing bad only: median(T) <= max(t), t being the parent's kzg_retrieve_blobs_bytes alone.  RTT_SHAPES="log_n:l:held:blobs,.."
overrides the shapes, RTT_CASES="none,one,eight,undecodable" the cases (RTT_APPEND=1 keeps the file's other rows); RTT_RESOURCES names the output of `hipcc -Rpass-analysis=kernel-resource-usage` over cosetbytes.hip, multilocate.hip and
recover.hip; RTT_BENCH / RTT_BENCH_PARENT name files with the flagship bench line of the session for this build and the parent's.  Writes
RTT_OUT (profiles/retrieve_tolerant.json) and renders profiles/retrieve_tolerant.md beside it (--render: render only)."""
import ctypes as C, hashlib, json, os, re, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.environ.get("RTT_OUT", os.path.join(ROOT, "profiles", "retrieve_tolerant.json"))
KERNELS = {"k_g1_decode_beILb0ELb0E": "k_g1_decode_be<device, one word>", "k_g1_decode_beILb1ELb0E": "k_g1_decode_be<wire, one word>",
           "k_g1_decode_beILb0ELb1E": "k_g1_decode_be<device, per item>", "k_fr_decode_beILb0E": "k_fr_decode_be<one word>", "k_fr_decode_beILb1E": "k_fr_decode_be<per item>",
           "k_mask_refused_weights": "k_mask_refused_weights", "k_coset_twist_rows": "k_coset_twist_rows", "k_coset_seg_sum": "k_coset_seg_sum",
           "k_locate_termsILi2E": "k_locate_terms<2>", "k_recover_scatterILb1E": "k_recover_scatter<bytes>"}


def fmt(c):
    return "–" if not c else "%.3f [%.3f, %.3f]" % (c["median"], c["min"], c["max"])


def render(doc):
    L = ["# Retrieving despite bad chunks (`kzg_retrieve_blobs_bytes_tolerant`): measured on one MI355X", "",
         "`python tools/time_retrieve_tolerant.py` (raw figures: `retrieve_tolerant.json`).  Host buffers in, host buffers out, evaluation form, one index row;",
         "one warm-up per route, then %d rounds with the routes taken in turns; **ms per call: median [min, max]**." % doc.get("reps", 0), "",
         "- **T** this library, `kzg_retrieve_blobs_bytes_tolerant`",
         "- **t** a build of the PARENT commit, loaded into the same process beside this library (its own context and SRS): `kzg_retrieve_blobs_bytes`; after a",
         "  reject the decode entries, `kzg_verify_multiproof_batch_locate` by blob and by item of the bad blobs, the good chunks reassembled on the host,",
         "  `kzg_recover_from_cosets_batch_bytes`; after a chunk that does not decode, that chunk dropped from every array and the call repeated.", "",
         "Before timing, T and t gave the same rows at every line.  The one rule is the project's own: with nothing bad and every held chunk used,",
         "median(T) ≤ max(t).  The lines with bad chunks have no threshold; they are what was measured.", "",
         "| n | l | B | held | used | bad chunks | T | t | T / t | pairing checks (T) | rule: median(T) ≤ max(t) |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc.get("rows", []):
        rule = "–" if r["case"] != "none" else ("yes" if r["T"]["median"] <= r["t"]["max"] else "**NO**")
        L.append("| 2^%d | %d | %d | %d | %d | %s | %s | %s | %.2f | %d | %s |" % (r["log_n"], r["chunk_len"], r["blobs"], r["held"], r["used"], r["case_text"], fmt(r["T"]), fmt(r["t"]),
                                                                            r["T"]["median"] / r["t"]["median"], r["checks"], rule))
    for name, key in (("this build", "bench"), ("the parent's build", "bench_parent")):
        if doc.get(key):
            L += ["", "Flagship bench line of the same session, %s: `%s`" % (name, doc[key])]
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
            cur = {"kernel": name} if name and not any(x["kernel"] == name for x in kernels) else None
            if cur:
                kernels.append(cur)
        elif cur is not None:
            cur[{"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
                 "LDS Size [bytes/block]": "lds"}[key]] = int(val)
    return sorted(kernels, key=lambda kk: kk["kernel"])


doc = json.load(open(OUT)) if os.path.exists(OUT) else {}
if os.environ.get("RTT_RESOURCES"):
    doc["kernels"] = take_resources(os.environ["RTT_RESOURCES"])
for env, key in (("RTT_BENCH", "bench"), ("RTT_BENCH_PARENT", "bench_parent")):
    if os.environ.get(env) and os.path.exists(os.environ[env]):
        lines = [ln.strip() for ln in open(os.environ[env]) if ln.strip().startswith("{")]
        if lines:
            doc[key] = lines[-1]
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
u64p, u8p, vp, sz, i32p, szp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_size_t)
B8 = lambda a: a.ctypes.data_as(u8p)                                                                # noqa: E731
REPS = int(os.environ.get("RTT_REPS", "7"))
DISTINCT = int(os.environ.get("RTT_DISTINCT", "2"))
CASES = os.environ.get("RTT_CASES", "none,one,eight,undecodable").split(",")
shapes = [[int(v) for v in s.split(":")] for s in os.environ.get("RTT_SHAPES", "16:64:513:64,20:16:65535:16").split(",")]
tau = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % bench.FR
ctx = k.Context(0)
srs = k.SRS.generate(tau, max(1 << (s[0] - 1) for s in shapes), ctx=ctx)
kz = k.KZG.new(ctx)

path = os.environ.get("RTT_BASELINE_LIB")
assert path and os.path.exists(path), "RTT_BASELINE_LIB must name the parent commit's library (tools/build_variant.sh)"
plib = C.CDLL(path)
plib.kzg_ctx_create.argtypes = [C.c_int32, C.POINTER(vp)]
plib.kzg_srs_generate.argtypes = [vp, u64p, C.c_uint64, sz, C.POINTER(vp)]
plib.kzg_coset_items_decode_be.argtypes = [vp, u8p, u8p, sz, sz, u64p, u64p, u64p, i32p]
plib.kzg_g1_decompress_be_device.argtypes = [vp, u8p, sz, u64p, u8p, u64p]
plib.kzg_verify_multiproof_batch_locate.argtypes = [vp, vp, u64p, sz, u64p, u64p, u64p, u64p, sz, sz, sz, u64p, u64p, u64p, sz, u8p, szp, szp]
plib.kzg_recover_from_cosets_batch_bytes.argtypes = [vp, u8p, u64p, sz, sz, sz, sz, sz, sz, C.c_int32, sz, u8p, i32p, u64p]
plib.kzg_retrieve_blobs_bytes.argtypes = [vp, vp, u8p, u64p, sz, u8p, u8p, sz, sz, sz, sz, sz, C.c_int32, sz, u64p, u64p, i32p, u8p, i32p, u64p, i32p]
pctx, psrs = vp(), vp()
assert plib.kzg_ctx_create(0, C.byref(pctx)) == 0
assert plib.kzg_srs_generate(pctx, P(k.fr.fr_from_int(tau)), 0, 4096, C.byref(psrs)) == 0      # the verifiers read l <= 64 of its points

rows = []
for log_n, l, held, B in shapes:
    n = 1 << log_n
    m, d = n // l, n // 2
    idx = np.array((list(range(0, m, 2)) + list(range(1, m, 2)))[:held], dtype=np.uint64)           # the even cosets first, then the odd ones
    count = len(idx)
    distinct = min(DISTINCT, B)
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
    ci, ki = np.repeat(np.arange(B, dtype=np.uint64), count), np.tile(idx, B)
    for case, case_text, n_bad in (("none", "0", 0), ("one", "1 fails its equation", 1), ("eight", "8 fail, in 8 blobs", 8), ("undecodable", "1 proof does not decode", 1)):
        if n_bad > B or case not in CASES:
            continue
        use = count if case == "none" else count - 1
        ys_be, pf_be = ys_good.copy(), pf_good.copy()
        bad_items = [(b * (B // max(n_bad, 1))) * count + (37 * (b + 1)) % count for b in range(n_bad)]
        for i in bad_items:
            if case == "undecodable":
                pf_be[32 * i] &= 0x3F                                                               # flag bits 0b00
            else:
                ys_be[32 * (i * l + 1) + 31] ^= 1
        out_T, out_t = np.zeros(B * n * 32, np.uint8), np.zeros(B * n * 32, np.uint8)
        flags_T, flags_t = np.zeros(B, np.int32), np.zeros(B, np.int32)
        ist, bst = np.zeros(N, np.uint8), np.zeros(B, np.uint8)
        nb, nu, checks = sz(0), sz(0), sz(0)
        ok, bad_index, bad_array = C.c_int32(0), C.c_uint64(0), C.c_int32(-1)
        words_y, words_p, words_c, inf_c = np.zeros((N, l, 4), np.uint64), np.zeros((N, 8), np.uint64), np.zeros((B, 8), np.uint64), np.zeros(B, np.uint8)

        def T():
            rc = lib.kzg_retrieve_blobs_bytes_tolerant(ctx.handle, srs.handle, B8(cm_be), P(idx), 1, B8(ys_be), B8(pf_be), B, count, use, n, l, 0, 1, 0, None, P(g2), B8(ist), B8(bst),
                                                       C.byref(nb), C.byref(nu), C.byref(checks), B8(out_T), flags_T.ctypes.data_as(i32p), None, None, None)
            assert rc == 0 and nu.value == 0 and nb.value == n_bad, (rc, nu.value, nb.value)

        def p_retrieve(rows_idx, index_rows, ys, pf, cnt, use_all=True):
            return plib.kzg_retrieve_blobs_bytes(pctx, psrs, B8(cm_be), P(rows_idx), index_rows, B8(ys), B8(pf), B, cnt, n, l, 0, 1, 0, None, P(g2), C.byref(ok), B8(out_t),
                                                 flags_t.ctypes.data_as(i32p), C.byref(bad_index), C.byref(bad_array))

        def recover_from(good):                                                                     # good: (B, count) bool; the first `use` good chunks of every blob, reassembled
            sel = np.stack([np.flatnonzero(good[b])[:use] for b in range(B)])
            flat = (sel + np.arange(B)[:, None] * count).reshape(-1)
            ys_sel = np.ascontiguousarray(ys_be.reshape(N, l * 32)[flat]).reshape(-1)
            rows_sel = np.ascontiguousarray(idx[sel.reshape(-1)].reshape(B, use))
            same = (sel == sel[0]).all()
            rc = plib.kzg_recover_from_cosets_batch_bytes(pctx, B8(ys_sel), P(rows_sel), 1 if same else B, B, use, n, l, 0, 1, 0, B8(out_t), flags_t.ctypes.data_as(i32p), None)
            assert rc == 0, rc

        def t():
            rc = p_retrieve(idx, 1, ys_be, pf_be, count)
            if case == "none":
                assert rc == 0 and ok.value == 1, (rc, ok.value)
                return
            if case == "undecodable":                                                               # the entry names the chunk; drop it from every blob's arrays and call again
                assert rc == _lib.ERR_DESERIALIZE and bad_array.value == 1, (rc, bad_array.value)
                b0, j0 = divmod(bad_index.value, count)
                keep = np.ones((B, count), bool)
                keep[b0, j0] = False
                for b in range(B):
                    if b != b0:
                        keep[b, count - 1] = False                                                  # one shape for all blobs: every blob gives up one chunk
                flat = np.flatnonzero(keep.reshape(-1))
                ys2 = np.ascontiguousarray(ys_be.reshape(N, l * 32)[flat]).reshape(-1)
                pf2 = np.ascontiguousarray(pf_be.reshape(N, 32)[flat]).reshape(-1)
                rows2 = np.ascontiguousarray(np.tile(idx, B)[flat].reshape(B, count - 1))
                rc = p_retrieve(rows2, B, ys2, pf2, count - 1)
                assert rc == 0 and ok.value == 1, (rc, ok.value)
                return
            assert rc == 0 and ok.value == 0, (rc, ok.value)
            assert plib.kzg_coset_items_decode_be(pctx, B8(ys_be), B8(pf_be), N, l, P(words_y), P(words_p), None, None) == 0
            assert plib.kzg_g1_decompress_be_device(pctx, B8(cm_be), B, P(words_c), B8(inf_c), None) == 0
            blob_ok = np.zeros(B, np.uint8)
            a, c2 = sz(0), sz(0)
            rc = plib.kzg_verify_multiproof_batch_locate(pctx, psrs, P(words_c), B, P(ci), P(ki), P(words_y), P(words_p), N, n, l, None, P(g2), P(ci), B, B8(blob_ok), C.byref(a),
                                                         C.byref(c2))
            assert rc == 0 and a.value == n_bad, (rc, a.value)
            bad_blobs = np.flatnonzero(blob_ok == 0)
            sub = (bad_blobs[:, None] * count + np.arange(count)[None, :]).reshape(-1)
            M2 = len(sub)
            sy, sp = np.ascontiguousarray(words_y[sub]), np.ascontiguousarray(words_p[sub])
            sci, ski, own = np.ascontiguousarray(ci[sub]), np.ascontiguousarray(ki[sub]), np.arange(M2, dtype=np.uint64)
            item_ok = np.zeros(M2, np.uint8)
            rc = plib.kzg_verify_multiproof_batch_locate(pctx, psrs, P(words_c), B, P(sci), P(ski), P(sy), P(sp), M2, n, l, None, P(g2), P(own), M2, B8(item_ok), C.byref(a), C.byref(c2))
            assert rc == 0 and a.value == n_bad, (rc, a.value)
            good = np.ones(N, bool)
            good[sub[item_ok == 0]] = False
            recover_from(good.reshape(B, count))

        for fn in (T, t):                                                                           # the warm-up, and the outputs to compare
            fn()
        if case == "undecodable":                                                                   # t recovered from count - 1 chunks, T from its first count - 1 good ones: the same blobs
            assert np.array_equal(out_T, out_t), "the routes differ"
        else:
            assert np.array_equal(out_T, out_t) and np.array_equal(flags_T, flags_t), "the routes differ"
        times = {"T": [], "t": []}
        for _ in range(REPS):
            for name, fn in (("T", T), ("t", t)):
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e3)
        row = {"log_n": log_n, "chunk_len": l, "blobs": B, "held": count, "used": use, "case": case, "case_text": case_text, "checks": int(checks.value),
               "value_bytes": B * count * l * 32, "distinct_blobs": distinct}
        for name, ts in times.items():
            row[name] = {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)

if os.environ.get("RTT_APPEND"):                                                                 # keep the file's other rows (a shape measured in a run of its own)
    done = {(r["log_n"], r["chunk_len"], r["case"]) for r in rows}
    rows = sorted([r for r in doc.get("rows", []) if (r["log_n"], r["chunk_len"], r["case"]) not in done] + rows, key=lambda r: r["log_n"])
doc["rows"], doc["reps"] = rows, REPS
json.dump(doc, open(OUT, "w"), indent=1)
render(doc)
