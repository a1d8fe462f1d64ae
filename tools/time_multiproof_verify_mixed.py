"""One mixed-shape call against a loop of per-shape calls: kzg_verify_multiproof_batch_mixed on this build, and kzg_verify_multiproof_batch once per
class on a build of the PARENT commit, per call from host buffers, derived weights on both sides.

Usage (GPU box):   MVM_PARENT_LIB=<the parent commit's libkzg_bn254_mi355x.so> python tools/time_multiproof_verify_mixed.py
                   python tools/time_multiproof_verify_mixed.py --render profiles/multiproof_verify_mixed.json     (the .md from the .json, no GPU)

The main process builds the items with this build (a known-tau SRS, KZG.compute_multiproofs) and writes them to a file; every timed configuration
is a fresh child process that loads ITS library through KZG_LIB_PATH with plain ctypes (the parent's library lacks the new entries, so the package
cannot load it), makes its own context and SRS of l_max points, and times MVM_REPS (9) calls after one warm-up:
  mixed          this build, one kzg_verify_multiproof_batch_mixed (item digests on the host pool: the entry has no device transcript)
  loop           the parent, one kzg_verify_multiproof_batch per class, the context's default transcript setting
  loop-host      the parent, the same loop with kzg_ctx_set_transcript_device(ctx, 1): item digests on the host, so that both sides hash alike
Each configuration runs once more under KZG_VB_TRACE=1 (the library then synchronises between phases; those times are not the reported ones) for
the share of the call that derives the weights.  Shapes:
  a   64 blobs x 64 chunks spread evenly over 8 classes, n = 2^10 .. 2^17, l = 16
  b   two classes of 32 768 items each: (2^16, 64) and (2^14, 16)
  c   one class of 65 536 x 64 at n = 2^16 (the blobs of b's first class, each coset twice)
The rule, for a and b: the mixed call's median must not lie above the max of the parent loop's own spread."""
import ctypes as C, hashlib, json, os, re, statistics, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.environ.get("MVM_OUT", os.path.join(ROOT, "profiles", "multiproof_verify_mixed.json"))
REPS = int(os.environ.get("MVM_REPS", "9"))
SHAPES = [s for s in os.environ.get("MVM_SHAPES", "a,b,c").split(",") if s]
FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617
TAU = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/srs/v1").digest(), "big") % FR
CONFIGS = ("mixed", "loop", "loop-host")
DESCRIBE = {"a": "64 blobs x 64 chunks over 8 classes, n = 2^10 .. 2^17, l = 16 (4 096 items)",
            "b": "two classes of 32 768 items: (2^16, 64) and (2^14, 16)",
            "c": "one class of 65 536 x 64, n = 2^16"}


def render(doc):
    L = ["# One mixed-shape call against a loop of per-shape calls", "",
         "`tools/time_multiproof_verify_mixed.py` on one MI355X, per call from host buffers, derived weights, median (min .. max) of %d calls after a warm-up, ms." % doc["reps"],
         "Every configuration is a process of its own with its own context and SRS.", "",
         "- **mixed**: this build, one `kzg_verify_multiproof_batch_mixed` (item digests on the host pool)",
         "- **loop**: the parent commit's library, one `kzg_verify_multiproof_batch` per class, the context's default transcript setting",
         "- **loop-host**: the same loop with `kzg_ctx_set_transcript_device(ctx, 1)`, so that both sides hash the items on the host", "",
         "| shape | items | classes | mixed | loop | loop-host | r_powers share: mixed / loop / loop-host |", "|---|---|---|---|---|---|---|"]
    f = lambda r: "%.3f (%.3f .. %.3f)" % (r["median_ms"], r["min_ms"], r["max_ms"])     # noqa: E731
    for s in doc["shapes"]:
        share = " / ".join("%.0f %%" % (100 * s[c]["r_powers_share"]) if s[c].get("r_powers_share") is not None else "-" for c in CONFIGS)
        L.append("| %s: %s | %d | %d | %s | %s | %s | %s |" % (s["shape"], DESCRIBE[s["shape"]], s["items"], s["classes"], f(s["mixed"]), f(s["loop"]), f(s["loop-host"]), share))
    L += ["", "The r_powers share is from `KZG_VB_TRACE=1` runs of their own (r_powers time over call time, both summed over the traced calls of the shape).", "",
          "## The rule", "", "For a and b the mixed call's median must not lie above the max of the parent loop's own spread."]
    for s in doc["shapes"]:
        if s["shape"] in "ab":
            for c in ("loop", "loop-host"):
                held = s["mixed"]["median_ms"] <= s[c]["max_ms"]
                L.append("- %s against %s: mixed median %.3f ms, loop max %.3f ms (median %.3f ms): **%s** (%.2fx the loop's median)."
                         % (s["shape"], c, s["mixed"]["median_ms"], s[c]["max_ms"], s[c]["median_ms"], "holds" if held else "DOES NOT HOLD", s["mixed"]["median_ms"] / s[c]["median_ms"]))
        else:
            L.append("- c (one shape, expected to lose to the uniform entry with device digests): mixed median %.3f ms against %.3f ms for the uniform call, %.2fx; "
                     "against the uniform call with host digests %.3f ms, %.2fx.  One-shape batches belong to `kzg_verify_multiproof_batch`."
                     % (s["mixed"]["median_ms"], s["loop"]["median_ms"], s["mixed"]["median_ms"] / s["loop"]["median_ms"], s["loop-host"]["median_ms"],
                        s["mixed"]["median_ms"] / s["loop-host"]["median_ms"]))
    with open(os.path.splitext(OUT)[0] + ".md", "w") as fh:
        fh.write("\n".join(L) + "\n")


if "--render" in sys.argv:
    OUT = sys.argv[sys.argv.index("--render") + 1]
    render(json.load(open(OUT)))
    sys.exit(0)

import numpy as np

u64p, vp, sz, i32 = C.POINTER(C.c_uint64), C.c_void_p, C.c_size_t, C.c_int32
P = lambda a: a.ctypes.data_as(u64p)     # noqa: E731


def child():
    """One configuration: MVM_CONFIG over every shape of the items file, the library of KZG_LIB_PATH.  One JSON line per shape."""
    config, items = os.environ["MVM_CONFIG"], np.load(os.environ["MVM_ITEMS"])
    lib = C.CDLL(os.environ["KZG_LIB_PATH"])
    lib.kzg_ctx_create.argtypes = [i32, C.POINTER(vp)]
    lib.kzg_srs_generate.argtypes = [vp, u64p, C.c_uint64, sz, C.POINTER(vp)]
    lib.kzg_ctx_set_transcript_device.argtypes = [vp, i32]
    lib.kzg_verify_multiproof_batch.argtypes = [vp, vp, u64p, sz, u64p, u64p, u64p, u64p, sz, sz, sz, u64p, u64p, C.POINTER(i32)]
    ctx = vp()
    assert lib.kzg_ctx_create(0, C.byref(ctx)) == 0
    if config == "loop-host":
        assert lib.kzg_ctx_set_transcript_device(ctx, 1) == 0
    if config == "mixed":
        lib.kzg_verify_multiproof_batch_mixed.argtypes = [vp, vp, u64p, sz, u64p, u64p, u64p, sz, u64p, u64p, u64p, u64p, sz, u64p, u64p, C.POINTER(i32)]
    tau_w = np.ascontiguousarray(items["tau_wire"])
    for shape in SHAPES:
        g = lambda name: np.ascontiguousarray(items["%s_%s" % (shape, name)])     # noqa: E731
        cn, cl, si, ki, ci, ys, pf, cm, g2 = (g(x) for x in ("cn", "cl", "si", "ki", "ci", "ys", "pf", "cm", "g2"))
        srs = vp()
        assert lib.kzg_srs_generate(ctx, P(tau_w), 0, int(cl.max()), C.byref(srs)) == 0
        ok = i32(0)
        if config == "mixed":
            def call():
                rc = lib.kzg_verify_multiproof_batch_mixed(ctx, srs, P(cm), len(cm), P(ci), P(cn), P(cl), len(cn), P(si), P(ki), P(ys), P(pf), len(si), None, P(g2), C.byref(ok))
                assert rc == 0 and ok.value == 1, (shape, rc, ok.value)
        else:
            # the split by shape is the caller's work today and is done ahead of the clock: per class its items, contiguous
            parts, off = [], np.concatenate([[0], np.cumsum(cl[si])]).astype(np.int64)
            for s in range(len(cn)):
                idx = np.nonzero(si == s)[0]
                if not len(idx):
                    continue
                l = int(cl[s])
                vals = np.ascontiguousarray(np.concatenate([ys[off[i]:off[i] + l] for i in idx]))
                used, local = np.unique(ci[idx], return_inverse=True)                   # the class's own commitments, its rows renumbered
                parts.append((np.ascontiguousarray(cm[used.astype(np.int64)]), np.ascontiguousarray(local.astype(np.uint64)), np.ascontiguousarray(ki[idx]), vals,
                              np.ascontiguousarray(pf[idx]), len(idx), int(cn[s]), l, np.ascontiguousarray(g2[s])))

            def call():
                for m_, c_, k_, v_, p_, n_items, n, l, g_ in parts:
                    rc = lib.kzg_verify_multiproof_batch(ctx, srs, P(m_), len(m_), P(c_), P(k_), P(v_), P(p_), n_items, n, l, None, P(g_), C.byref(ok))
                    assert rc == 0 and ok.value == 1, (shape, n, l, rc, ok.value)
        call()
        ms = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        sys.stderr.flush()
        print(json.dumps({"shape": shape, "config": config, "items": int(len(si)), "classes": int(len(set(si.tolist()))), "median_ms": statistics.median(ms), "min_ms": min(ms),
                          "max_ms": max(ms), "all_ms": ms}), flush=True)
        sys.stderr.write("MVM_SHAPE_END %s\n" % shape)
        sys.stderr.flush()


if "--child" in sys.argv:
    child()
    sys.exit(0)


def build_items(path):
    import rust_kzg_bn254_amd as k
    ctx = k.Context(0)
    srs = k.SRS.generate(TAU, 1 << 17, ctx=ctx)
    rng = np.random.default_rng(2024)
    out = {"tau_wire": k.fr.fr_from_int(TAU)}
    g2_at = lambda l: k.helpers.g2_mul_generator(k.fr.fr_from_int(pow(TAU, l, FR)))     # noqa: E731

    def blob(n, l):
        ev = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
        ev[:, 3] &= np.uint64((1 << 60) - 1)                                            # any words below r are a field element in wire form
        kz = k.KZG.new(ctx)
        kz.calculate_and_store_roots_of_unity(n * 32)
        poly = k.PolynomialEvalForm(ev)
        return kz.commit_eval_form(poly, srs), kz.cosets(poly, l), kz.compute_multiproofs(poly, srs, l)

    def pack(shape, classes, blobs):
        """blobs: (class, commitment, cosets, proofs, coset indices) in item order"""
        si, ki, ci, ys, pf, cm = [], [], [], [], [], []
        for b, (s, c, co, pr, ks) in enumerate(blobs):
            cm.append(c)
            for kk in ks:
                si.append(s); ki.append(kk); ci.append(b); ys.append(co[kk]); pf.append(pr[kk])
        out.update({shape + "_cn": np.array([c[0] for c in classes], np.uint64), shape + "_cl": np.array([c[1] for c in classes], np.uint64),
                    shape + "_si": np.array(si, np.uint64), shape + "_ki": np.array(ki, np.uint64), shape + "_ci": np.array(ci, np.uint64),
                    shape + "_ys": np.concatenate(ys), shape + "_pf": np.stack(pf), shape + "_cm": np.stack(cm),
                    shape + "_g2": np.stack([g2_at(l) for _, l in classes])})

    if "a" in SHAPES:
        classes = [(1 << e, 16) for e in range(10, 18)]
        blobs = []
        for j in range(64):                                                              # blob j has class j mod 8: the shapes arrive interleaved
            n, l = classes[j % 8]
            c, co, pr = blob(n, l)
            blobs.append((j % 8, c, co, pr, [int(v) for v in rng.choice(n // l, 64, replace=False)]))
        pack("a", classes, blobs)
    big = None
    if "b" in SHAPES or "c" in SHAPES:
        big = [blob(1 << 16, 64) for _ in range(32)]                                     # 32 x 1 024 cosets
    if "b" in SHAPES:
        classes = [(1 << 16, 64), (1 << 14, 16)]
        small = [blob(1 << 14, 16) for _ in range(32)]
        blobs = []
        for j in range(32):
            blobs.append((0, *big[j], list(range(1024))))
            blobs.append((1, *small[j], list(range(1024))))
        pack("b", classes, blobs)
    if "c" in SHAPES:
        pack("c", [(1 << 16, 64)], [(0, *big[j], list(range(1024)) * 2) for j in range(32)])
    np.savez(path, **out)


def run_config(config, items, trace):
    lib = os.path.join(ROOT, "rust-kzg-bn254_amd", "libkzg_bn254_mi355x.so") if config == "mixed" else os.environ["MVM_PARENT_LIB"]
    env = dict(os.environ, KZG_LIB_PATH=lib, MVM_CONFIG=config, MVM_ITEMS=items, MVM_REPS=str(5 if trace else REPS))
    env.pop("KZG_VB_TRACE", None)
    if trace:
        env["KZG_VB_TRACE"] = "1"
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, (config, res.stdout[-2000:], res.stderr[-3000:])
    rows = {}
    for ln in res.stdout.splitlines():
        if ln.startswith("{"):
            r = json.loads(ln)
            rows[r["shape"]] = r
    if trace:                                                                            # per shape: r_powers and call times of every traced line
        for shape, text in zip(SHAPES, res.stderr.split("MVM_SHAPE_END")):
            rp = [float(m.group(1)) for m in re.finditer(r"r_powers[^:,]*?(?: \([^)]*\))? ([0-9.]+) ms", text)]
            call = [float(m.group(1)) for m in re.finditer(r"call ([0-9.]+) ms", text)]
            rows[shape]["r_powers_share"] = (sum(rp) / sum(call)) if call and len(rp) == len(call) else None
    return rows


def main():
    assert os.path.exists(os.environ.get("MVM_PARENT_LIB", "")), "MVM_PARENT_LIB must name the parent commit's library"
    with tempfile.TemporaryDirectory() as tmp:
        items = os.path.join(tmp, "items.npz")
        build_items(items)
        doc = {"tool": "tools/time_multiproof_verify_mixed.py", "reps": REPS, "shapes": []}
        timed = {c: run_config(c, items, False) for c in CONFIGS}
        traced = {c: run_config(c, items, True) for c in CONFIGS}
    for shape in SHAPES:
        row = {"shape": shape, "items": timed["mixed"][shape]["items"], "classes": timed["mixed"][shape]["classes"]}
        for c in CONFIGS:
            row[c] = {kk: timed[c][shape][kk] for kk in ("median_ms", "min_ms", "max_ms", "all_ms")}
            row[c]["r_powers_share"] = traced[c][shape].get("r_powers_share")
        doc["shapes"].append(row)
        print(json.dumps({kk: (vv if not isinstance(vv, dict) else {q: vv[q] for q in ("median_ms", "min_ms", "max_ms", "r_powers_share")}) for kk, vv in row.items()}), flush=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    render(doc)


if __name__ == "__main__":
    main()
