"""CPU: the host side of `kzg_recover_from_cosets_batch` (csrc/host_recover.h RecoverBatchPlan) as a plain g++ program built with
AddressSanitizer and UBSan and run on its own, no GPU and no library: the error table in its documented order, the deduplication of
missing sets into patterns, `pattern_of` and `item_of`, the group sizes over a grid of (shape, budget, blobs) with the ragged last group
and the budget too small for one blob, the word layout and what one upload carries (tests/hostcheck/recoverbatchcheck.cpp states each
check).  Plus the ABI surface: the three new exports with their declared signatures, and the pure query without a context."""
import ctypes as C
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
NAMES = ("kzg_recover_from_cosets_batch", "kzg_ctx_set_recover_group_bytes", "kzg_recover_batch_info")


def test_recover_batch_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "recoverbatchcheck")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(HERE, "hostcheck", "recoverbatchcheck.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "recoverbatchcheck ok", (r.stdout[-500:], r.stderr[-3000:])


def test_host_recover_header_and_what_it_includes_have_no_hip():
    for name in ("host_recover.h", "ntt_plan.h", "host_log2.h"):
        src = open(os.path.join(CSRC, name)).read()
        includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
        assert not any("hip" in inc for inc in includes), (name, includes)


def test_the_new_exports_exist_with_their_declared_signatures():
    import rust_kzg_bn254_amd as k
    L = k._lib
    lib = L.load()                                                     # loading needs no GPU
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read(), flags=re.S)
    ctype = {"kzg_ctx*": L.vp, "const uint64_t*": L.u64p, "uint64_t*": L.u64p, "int32_t*": C.POINTER(L.i32), "size_t": L.sz, "int32_t": L.i32,
             "kzg_recover_batch_info_t*": L.vp}
    for name in NAMES:
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name + " is not declared in the header"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        types = [re.sub(r"\s*\w+$", "", p).replace(" *", "*") for p in params]      # drop the parameter's name
        res, args = L.PROTOTYPES[name]
        assert res is L.i32 and [ctype[t] for t in types] == args, (name, types)
        assert hasattr(lib, name), name + " is not exported"
    assert C.sizeof(L.RecoverBatchInfo) == 32
    m = re.search(r"typedef struct kzg_recover_batch_info_t \{(.*?)\}", header, flags=re.S)
    fields = [ln.split()[-1].rstrip(";") for ln in m.group(1).splitlines() if ln.strip()]
    assert fields == [f[0] for f in L.RecoverBatchInfo._fields_], fields
    hpp = open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.hpp")).read()
    assert "kzg_recover_from_cosets_batch(" in hpp


def test_the_query_runs_without_a_context_and_returns_the_shape_errors():
    import rust_kzg_bn254_amd as k
    L = k._lib
    lib = L.load()
    info = k.helpers.recover_batch_info(7, 8, 64, 4)
    assert info["blobs_per_group"] == 7 and info["groups"] == 1 and info["group_bytes"] == 7 * info["blob_bytes"] + 16
    per = info["blob_bytes"]
    assert per >= 2 * 64 * 32
    three = k.helpers.recover_batch_info(7, 8, 64, 4, group_bytes=3 * per)
    assert (three["blobs_per_group"], three["groups"], three["group_bytes"]) == (3, 3, 3 * per + 16)
    assert k.helpers.recover_batch_info(7, 8, 64, 4, group_bytes=3 * per + per - 1)["blobs_per_group"] == 3
    assert k.helpers.recover_batch_info(7, 8, 64, 4, group_bytes=4 * per)["blobs_per_group"] == 4
    one = k.helpers.recover_batch_info(7, 8, 64, 4, group_bytes=1)                   # too small for one blob: groups of one
    assert (one["blobs_per_group"], one["groups"]) == (1, 7)
    assert k.helpers.recover_batch_info(100000, 8, 64, 4)["blobs_per_group"] == 32768          # grid.y
    out = L.RecoverBatchInfo()

    def q(blobs=7, count=8, n=64, l=4, out_len=0, out_=C.byref(out)):
        return lib.kzg_recover_batch_info(blobs, count, n, l, out_len, 0, out_)

    assert q(out_=None) == L.ERR_INVALID_ARG and q(blobs=0, n=0) == L.ERR_INVALID_ARG
    assert q(n=0) == L.ERR_NOT_POWER_OF_TWO and q(n=96) == L.ERR_NOT_POWER_OF_TWO
    assert q(n=1 << 25, l=3) == L.ERR_DOMAIN
    assert q(l=3) == L.ERR_INVALID_ARG and q(l=64) == L.ERR_INVALID_ARG and q(count=0) == L.ERR_INVALID_ARG and q(count=17) == L.ERR_INVALID_ARG
    assert q(out_len=65) == L.ERR_INVALID_ARG and q(out_len=64) == 0 and q(out_len=32) == 0
    assert q(count=1, n=1 << 24, l=1) == L.ERR_TOO_LARGE
    assert q(blobs=2 ** 64 // (64 * 32) + 1) == L.ERR_INVALID_ARG
    with pytest.raises(k.errors.GenericError):
        k.helpers.recover_batch_info(7, 8, 96, 4)
