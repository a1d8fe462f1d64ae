"""Host-only (no GPU): the retriever's serialized form.  tests/hostcheck/recoverbytescheck.cpp compiles csrc/g1_decode.h and
csrc/host_recover.h for the host with the bound-checked field (-DKZG_BOUND_CHECK: every lazy-reduction bound is an abort()) and checks
`fr_encode_wire_to_be` against `fr_decode_be_to_wire` and against a second implementation, then walks `recover_bytes_check` through its
table.  A stand-alone program with its own main: it runs once as it is and once under AddressSanitizer + UndefinedBehaviorSanitizer, as
a subprocess; nothing is loaded into Python under a sanitizer.  Plus the ABI surface of the two new entries."""
import ctypes as C
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
SRC = os.path.join(HERE, "hostcheck", "recoverbytescheck.cpp")
NAMES = ("kzg_recover_from_cosets_batch_bytes", "kzg_retrieve_blobs_bytes")


def _build_and_run(exe, extra, env=None):
    subprocess.check_call(["g++", "-std=c++17", "-DKZG_BOUND_CHECK", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", *extra, "-I" + CSRC, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "recoverbytescheck ok", (r.stdout[-500:], r.stderr[-3000:])


def test_codec_and_argument_checks(tmp_path):
    _build_and_run(str(tmp_path / "recoverbytescheck"), ["-O1"])


def test_the_same_program_under_asan_ubsan(tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    _build_and_run(str(tmp_path / "recoverbytescheck_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"], env)


def test_the_new_exports_exist_with_their_declared_signatures():
    import rust_kzg_bn254_amd as k
    L = k._lib
    lib = L.load()                                                     # loading needs no GPU
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read(), flags=re.S)
    ctype = {"kzg_ctx*": L.vp, "const kzg_srs*": L.vp, "const uint64_t*": L.u64p, "uint64_t*": L.u64p, "const uint8_t*": L.u8p, "uint8_t*": L.u8p,
             "int32_t*": C.POINTER(L.i32), "size_t": L.sz, "int32_t": L.i32}
    for name in NAMES:
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name + " is not declared in the header"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        types = [re.sub(r"\s*\w+$", "", p).replace(" *", "*") for p in params]      # drop the parameter's name
        res, args = L.PROTOTYPES[name]
        want = [ctype[t] for t in types]
        assert res is L.i32 and len(want) == len(args), (name, types)
        for w, a in zip(want, args):                                   # (uint64_t* outputs are POINTER(c_uint64) under either name)
            assert w is a or (w is L.u64p and a._type_ is C.c_uint64), (name, types)
        assert hasattr(lib, name), name + " is not exported"
    assert hasattr(k.KZG, "recover_from_cosets_batch_bytes") and hasattr(k.verifier, "retrieve_blobs_bytes")


def test_null_and_shape_errors_need_no_device():
    import rust_kzg_bn254_amd as k
    L = k._lib
    lib = L.load()
    assert lib.kzg_recover_from_cosets_batch_bytes(None, None, None, 1, 1, 1, 64, 4, 0, 0, 0, None, None, None) == L.ERR_INVALID_ARG
    assert lib.kzg_retrieve_blobs_bytes(None, None, None, None, 1, None, None, 1, 1, 64, 4, 0, 0, 0, None, None, None, None, None, None, None) == L.ERR_INVALID_ARG
