"""CPU: the host side of `kzg_prove_cosets` (csrc/host_prove_cosets.h) as a plain g++ program, no GPU and no library, built once plain
and once with AddressSanitizer and UBSan and run on its own both times: the argument table in its documented order, group sizes
monotone in the budget and never 0, S, the segments and the levels with the per-lane bound on dependent products, and a host model of
the three passes (the kernels' index arithmetic on host_fr.h, on buffers of exactly the planned sizes) against the sequential
recurrence for a grid of (d, l, S, k) that reaches five levels (tests/hostcheck/provecosetscheck.cpp states each check), and the plans of
a small grid pinned in tests/golden/prove_cosets_plans.txt (recorded from that program when the prover was added; a change of policy
re-records the lines it means to change and no others).  Plus the ABI surface: the three exports with their declared signatures."""
import ctypes as C
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
SRC = os.path.join(HERE, "hostcheck", "provecosetscheck.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan+ubsan"])
def test_plans_keep_their_checks_and_equal_the_pinned_table(tmp_path, flags):
    exe = str(tmp_path / "provecosetscheck")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I" + CSRC, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    got = r.stdout.splitlines()
    assert got and got[-1] == "provecosetscheck ok"
    want = open(os.path.join(HERE, "golden", "prove_cosets_plans.txt")).read().splitlines()
    assert len(got) - 1 == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d" % (i + 1)
    # the pinned grid reaches one segment, several, two carry levels, a short S, several groups, and both sides of the single-item rule
    text = "\n".join(want)
    for piece in (" levels=64/1 ", " levels=2048/32,32/1 ", " levels=65536/1024,1024/16,16/1 ", " S=8 ", " groups=100 ", " groups=1 ", " items=1 ", " single=0"):
        assert piece in text, piece


def test_the_host_header_includes_no_hip():
    for name in ("host_prove_cosets.h", "host_encode.h", "host_fr.h"):
        src = open(os.path.join(CSRC, name)).read()
        assert not any("hip" in ln for ln in src.splitlines() if ln.startswith("#include")), name


def test_the_new_exports_exist_with_their_declared_signatures():
    import rust_kzg_bn254_amd as k
    L = k._lib
    lib = L.load()                                                     # loading needs no GPU
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read(), flags=re.S)
    ctype = {"kzg_ctx*": L.vp, "kzg_srs*": L.vp, "const uint64_t*": L.u64p, "uint64_t*": L.u64p, "uint8_t*": L.u8p, "size_t": L.sz, "int32_t": L.i32,
             "kzg_prove_cosets_info_t*": L.vp}
    for name in ("kzg_prove_cosets", "kzg_coset_quotients", "kzg_prove_cosets_info"):
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name + " is not declared in the header"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        types = [re.sub(r"\s*\w+$", "", p).replace(" *", "*") for p in params]      # drop the parameter's name
        res, args = L.PROTOTYPES[name]
        assert res is L.i32 and [ctype[t] for t in types] == args, (name, types)
        assert hasattr(lib, name), name + " is not exported"
    # the struct of the query: the header's layout is the binding's
    assert C.sizeof(L.ProveCosetsInfo) == 56
    m = re.search(r"typedef struct kzg_prove_cosets_info_t \{(.*?)\}", header, flags=re.S)
    fields = [ln.split()[-1].rstrip(";") for ln in m.group(1).splitlines() if ln.strip()]
    assert fields == [f[0] for f in L.ProveCosetsInfo._fields_], fields
    # the query runs without a context
    info = k.helpers.prove_cosets_info(1 << 14, 1 << 15, 1, 40)
    assert info["items_per_group"] == 40 and info["groups"] == 1 and info["seg_len"] == 64 and info["segments"] == 256 and info["carry_levels"] == 2
    assert info["launches"] == 5 and info["group_bytes"] == 40 * info["item_bytes"]
    # the argument errors that need no GPU
    null = lib.kzg_prove_cosets(None, None, None, 1, 64, 0, 128, 1, None, None, 0, None, None, None, None)
    assert null == L.ERR_INVALID_ARG and lib.kzg_coset_quotients(None, None, 1, 64, 0, 128, 1, None, None, 0, None, None, None) == L.ERR_INVALID_ARG
