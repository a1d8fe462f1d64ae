"""Host-only (no GPU): the retriever's call that survives bad chunks and the located verifier on bytes.
tests/hostcheck/retrievetolerantcheck.cpp compiles csrc/host_locate.h and csrc/host_recover.h with g++ and checks the subset plan against a
brute-force plan, the choice of the first use_count good items, the planner of the recovery from chosen items against `recover_batch_plan`,
and the argument table of `kzg_retrieve_blobs_bytes_tolerant` in its order.  A stand-alone program with its own main: it runs once as it is
and once under AddressSanitizer + UndefinedBehaviorSanitizer, as a subprocess; nothing is loaded into Python under a sanitizer.  Plus the
ABI surface of the two new entries and their errors that need no device."""
import ctypes as C
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
SRC = os.path.join(HERE, "hostcheck", "retrievetolerantcheck.cpp")
NAMES = ("kzg_verify_multiproof_batch_locate_bytes", "kzg_retrieve_blobs_bytes_tolerant")


def _build_and_run(exe, extra, env=None):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", *extra, "-I" + CSRC, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "retrievetolerantcheck ok", (r.stdout[-500:], r.stderr[-3000:])


def test_plans_choice_and_argument_table(tmp_path):
    _build_and_run(str(tmp_path / "retrievetolerantcheck"), ["-O1"])


def test_the_same_program_under_asan_ubsan(tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    _build_and_run(str(tmp_path / "retrievetolerantcheck_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"], env)


def test_the_new_exports_exist_with_their_declared_signatures():
    import rust_kzg_bn254_amd as k
    L = k._lib
    lib = L.load()                                                     # loading needs no GPU
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read(), flags=re.S)
    ctype = {"kzg_ctx*": L.vp, "kzg_srs*": L.vp, "const uint64_t*": L.u64p, "uint64_t*": L.u64p, "const uint8_t*": L.u8p, "uint8_t*": L.u8p,
             "int32_t*": C.POINTER(L.i32), "size_t*": C.POINTER(L.sz), "size_t": L.sz, "int32_t": L.i32}
    for name in NAMES:
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name + " is not declared in the header"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        types = [re.sub(r"\s*\w+$", "", p).replace(" *", "*") for p in params]      # drop the parameter's name
        res, args = L.PROTOTYPES[name]
        want = [ctype[t] for t in types]
        assert res is L.i32 and len(want) == len(args), (name, types)
        for w, a in zip(want, args):                                   # (pointer types are compared by what they point to)
            assert w is a or (hasattr(w, "_type_") and hasattr(a, "_type_") and w._type_ is a._type_), (name, types)
        assert hasattr(lib, name), name + " is not exported"
    assert hasattr(k.verifier, "locate_bad_multiproofs_bytes") and hasattr(k.verifier, "retrieve_blobs_bytes_tolerant")


def test_null_and_shape_errors_need_no_device():
    import rust_kzg_bn254_amd as k
    L = k._lib
    lib = L.load()
    sz = L.sz
    assert lib.kzg_verify_multiproof_batch_locate_bytes(None, None, None, 0, None, None, None, None, 0, 64, 4, None, None, None, 0, None, None, None, None, None,
                                                        None) == L.ERR_INVALID_ARG
    idx = (C.c_uint64 * 2)(0, 1)
    ys, pf, cm = (C.c_uint8 * (2 * 4 * 32))(), (C.c_uint8 * 64)(), (C.c_uint8 * 32)()
    st, bs, polys = (C.c_uint8 * 2)(), (C.c_uint8 * 1)(), (C.c_uint8 * (64 * 32))()
    a, b = sz(0), sz(0)

    def call(ctx_like, item_status=st, blob_status=bs, bad_items=C.byref(a), unrecovered=C.byref(b), use=2, count=2, n=64, l=4):
        return lib.kzg_retrieve_blobs_bytes_tolerant(ctx_like, None, cm, idx, 1, ys, pf, 1, count, use, n, l, 0, 1, 0, None, None, item_status, blob_status, bad_items,
                                                     unrecovered, None, polys, None, None, None, None)
    assert call(None) == L.ERR_INVALID_ARG                               # a null context in front of everything
    # every other row of the recovery's table is decided before the context is touched: a context that is not null is never dereferenced here
    fake = C.c_void_p(1)
    assert call(fake, item_status=None) == L.ERR_INVALID_ARG and call(fake, blob_status=None) == L.ERR_INVALID_ARG
    assert call(fake, bad_items=None) == L.ERR_INVALID_ARG and call(fake, unrecovered=None) == L.ERR_INVALID_ARG
    assert call(fake, n=96) == L.ERR_NOT_POWER_OF_TWO and call(fake, n=1 << 25) == L.ERR_DOMAIN
    assert call(fake, use=0) == L.ERR_INVALID_ARG and call(fake, use=3) == L.ERR_INVALID_ARG and call(fake, count=17, use=2) == L.ERR_INVALID_ARG
    assert call(fake, l=3) == L.ERR_INVALID_ARG
