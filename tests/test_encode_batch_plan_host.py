"""CPU: the host side of `kzg_encode_cosets_batch` (csrc/host_encode.h EncodeBatchPlan, csrc/g1fft_plan.h with a batch) as a plain g++
program, no GPU and no library, built once plain and once with AddressSanitizer and UBSan and run on its own both times: the error
table in its documented order with the two new rows, batch = 1 giving the plans of a single transform field for field, group sizes
monotone in the budget and never 0, the bytes a group reserves against the highest index every launch addresses, the model's lanes
against the grids (tests/hostcheck/encodebatchcheck.cpp states each check), and the plans of a small (shape, B) grid pinned in
tests/golden/encode_batch_plans.txt (recorded from that program when the batched encoder was added; a change of policy re-records the
lines it means to change and no others).  Plus the ABI surface: the three new exports with their declared signatures."""
import ctypes as C
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
SRC = os.path.join(HERE, "hostcheck", "encodebatchcheck.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan+ubsan"])
def test_batch_plans_keep_their_checks_and_equal_the_pinned_table(tmp_path, flags):
    exe = str(tmp_path / "encodebatchcheck")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I" + CSRC, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    got = r.stdout.splitlines()
    assert got and got[-1] == "encodebatchcheck ok"
    want = open(os.path.join(HERE, "golden", "encode_batch_plans.txt")).read().splitlines()
    assert len(got) - 1 == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d" % (i + 1)
    # the pinned grid reaches both forms on lanes and on pairs, the padding copy and the spread load, several groups, and the rule
    text = "\n".join(want)
    for piece in (" direct[", " direct_pairs[", " radix2[", " radix2_pairs[", " pad[", " spread[", " gather[", " gather_bitrev[", " groups=3 ", " groups=7 ", " batched=0 "):
        assert piece in text, piece


def test_host_headers_of_the_batch_plan_include_no_hip():
    for name in ("host_encode.h", "g1fft_plan.h", "ntt_plan.h"):
        src = open(os.path.join(CSRC, name)).read()
        assert not any("hip" in ln for ln in src.splitlines() if ln.startswith("#include")), name


def test_the_new_exports_exist_with_their_declared_signatures():
    import rust_kzg_bn254_amd as k
    L = k._lib
    lib = L.load()                                                     # loading needs no GPU
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read(), flags=re.S)
    ctype = {"kzg_ctx*": L.vp, "kzg_srs*": L.vp, "const uint64_t*": L.u64p, "uint64_t*": L.u64p, "uint8_t*": L.u8p, "size_t": L.sz, "int32_t": L.i32,
             "kzg_encode_batch_info*": L.vp}
    for name in ("kzg_encode_cosets_batch", "kzg_ctx_set_encode_group_bytes", "kzg_encode_cosets_batch_info"):
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name + " is not declared in the header"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        types = [re.sub(r"\s*\w+$", "", p).replace(" *", "*") for p in params]      # drop the parameter's name
        res, args = L.PROTOTYPES[name]
        assert res is L.i32 and [ctype[t] for t in types] == args, (name, types)
        assert hasattr(lib, name), name + " is not exported"
    # the structs of the query: the header's layout is the binding's
    assert C.sizeof(L.EncodeTransformInfo) == 16 and C.sizeof(L.EncodeBatchInfo) == 64
    m = re.search(r"typedef struct kzg_encode_batch_info \{(.*?)\}", header, flags=re.S)
    fields = [ln.split()[-1].rstrip(";") for ln in m.group(1).splitlines() if ln.strip()]
    assert fields == [f[0] for f in L.EncodeBatchInfo._fields_], fields
    m = re.search(r"typedef struct kzg_encode_transform_info \{(.*?)\}", header, flags=re.S)
    fields = [ln.split()[-1].rstrip(";") for ln in m.group(1).splitlines() if ln.strip()]
    assert fields == [f[0] for f in L.EncodeTransformInfo._fields_], fields
    # the query runs without a context
    info = k.helpers.encode_batch_info(256, 2048, 16, 7)
    assert info["blobs_per_group"] == 7 and info["groups"] == 1 and info["batched"] and info["forward"]["load"] == "pad"
