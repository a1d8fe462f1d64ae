"""CPU-only checks of locating the bad headers of a batch (`kzg_header_group_sums`, `kzg_verify_length_proof_batch_locate`):
csrc/host_header_locate.h as a plain g++ program (tests/hostcheck/headerlocatecheck.cpp states each check: the composite keys and the
plan of the 2 count G2 points against a naive grouping, the assembly of the components, the error table in its order, the search over
a stand-in group with planted bad headers and its bound on the checks), built once plainly and once with AddressSanitizer and UBSan;
the declarations of the two entries; the argument errors that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pyref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
ENTRIES = ("kzg_header_group_sums", "kzg_verify_length_proof_batch_locate")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_host_header_locate_as_a_host_program(tmp_path, flags):
    """A stand-alone binary with its own main, run directly (no preloaded runtime)."""
    exe = str(tmp_path / "headerlocatecheck")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I" + CSRC,
                           os.path.join(HERE, "hostcheck", "headerlocatecheck.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "headerlocatecheck ok", (r.stdout[-500:], r.stderr[-3000:])


def test_host_header_locate_header_includes_no_hip():
    src = open(os.path.join(CSRC, "host_header_locate.h")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert '"host_locate.h"' in includes and not any("hip" in inc or "engine" in inc for inc in includes), includes
    assert "kzg_ctx" not in src.replace("no kzg_ctx", "")


def test_header_prototypes_and_exports_agree_on_the_two_entries():
    import rust_kzg_bn254_amd as k
    hdr = open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read()
    lib = C.CDLL(k._lib.LIB_PATH)
    L = k._lib
    params = {}
    for name in ENTRIES:
        decl = re.search(r"\bint32_t %s\s*\(([^;]*)\);" % name, hdr)
        assert decl, name
        assert name in L.PROTOTYPES and hasattr(lib, name), name
        params[name] = [re.sub(r"/\*.*?\*/", "", p).split()[-1].lstrip("*") for p in decl.group(1).split(",")]
        assert len(params[name]) == len(L.PROTOTYPES[name][1]), name
    batch = L.PROTOTYPES["kzg_verify_length_proof_batch"][1]
    szp, u64ptr = C.POINTER(L.sz), C.POINTER(C.c_uint64)
    # the batch entry's inputs (everything in front of out_ok), then the partition, the outputs and bad_index
    assert L.PROTOTYPES["kzg_header_group_sums"] == (L.i32, batch[:10] + [L.u64p, L.sz, L.u64p, L.u8p, L.u64p, L.u64p, u64ptr])
    assert L.PROTOTYPES["kzg_verify_length_proof_batch_locate"] == (L.i32, batch[:10] + [L.u64p, L.sz, L.u8p, szp, szp, u64ptr])
    head = ["ctx", "commitments_xy", "length_commitments", "length_proofs", "claimed_lens", "count", "shift_lens", "g1_tau_shifts_xy", "n_shifts", "weights_mont",
            "group_indices", "n_groups"]
    assert params["kzg_header_group_sums"] == head + ["out_u_xy", "out_u_is_infinity", "out_w_g2", "out_pi_g2", "bad_index"]
    assert params["kzg_verify_length_proof_batch_locate"] == head + ["out_group_ok", "out_bad_groups", "out_pairing_checks", "bad_index"]


def test_the_docstrings_point_to_the_new_entry():
    from rust_kzg_bn254_amd import verifier
    hdr = open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read()
    assert "bisect" not in verifier.verify_length_proof_batch.__doc__ and "locate_bad_headers" in verifier.verify_length_proof_batch.__doc__
    assert "(bisection)" not in hdr


def test_argument_errors_that_need_no_device():
    """The null context is the first check of both entries, as it is of the batch entry: every call below returns before it needs a
    device, and writes no output.  The rest of the table needs a context (tests/test_gpu_header_locate.py).  The Python surface refuses
    its own argument errors without creating a context."""
    import rust_kzg_bn254_amd as k
    from rust_kzg_bn254_amd import verifier
    lib = k.load()
    L = k._lib
    g1 = np.zeros((1, 8), np.uint64)
    g2 = np.zeros((1, 16), np.uint64)
    lens = np.array([4], np.uint64)
    idx = np.zeros(1, np.uint64)
    w = pyref.frs_to_mont([1, 1])
    out1, out2 = np.full((1, 8), 7, np.uint64), np.full((1, 16), 7, np.uint64)
    flag = np.full(1, 7, np.uint8)
    n_bad, checks, bad = L.sz(7), L.sz(7), C.c_uint64(7)
    u8 = lambda a: a.ctypes.data_as(L.u8p)                                      # noqa: E731
    P = L.ptr
    assert lib.kzg_header_group_sums(None, P(g1), P(g2), P(g2), P(lens), 1, P(lens), P(g1), 1, P(w), P(idx), 1, P(out1), u8(flag), P(out2), P(out2),
                                     C.byref(bad)) == L.ERR_INVALID_ARG
    assert lib.kzg_header_group_sums(None, None, None, None, None, 0, None, None, 0, None, None, 0, None, None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.kzg_verify_length_proof_batch_locate(None, P(g1), P(g2), P(g2), P(lens), 1, P(lens), P(g1), 1, P(w), P(idx), 1, u8(flag), C.byref(n_bad),
                                                    C.byref(checks), C.byref(bad)) == L.ERR_INVALID_ARG
    assert lib.kzg_verify_length_proof_batch_locate(None, None, None, None, None, 0, None, None, 0, None, None, 0, None, None, None, None) == L.ERR_INVALID_ARG
    assert (out1 == 7).all() and (out2 == 7).all() and flag[0] == 7 and (n_bad.value, checks.value, bad.value) == (7, 7, 7)
    before = dict(L._default_ctx)                                               # device id -> Context: must not grow
    G = k.errors.GenericError
    shifts = {4: g1[0]}
    with pytest.raises(k.errors.InvalidInputLength):
        verifier.locate_bad_headers(g1, np.zeros((2, 16), np.uint64), g2, [4], shifts)
    with pytest.raises(k.errors.InvalidInputLength):
        verifier.locate_bad_headers(g1, g2, g2, [4], shifts, weights=pyref.frs_to_mont([1]))
    with pytest.raises(G, match="not the same"):
        verifier.locate_bad_headers(g1, g2, g2, [4], shifts, groups=[0, 0], n_groups=1)
    with pytest.raises(G, match="n_groups"):
        verifier.header_group_sums(g1, g2, g2, [4], shifts, groups=[0])
    with pytest.raises(G, match="item"):
        verifier.header_group_sums(g1, g2, g2, [4], shifts, groups="commitment")
    assert L._default_ctx == before
