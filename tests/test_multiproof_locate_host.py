"""CPU-only checks of locating the bad groups of a batch of coset proofs (`kzg_coset_group_sums`, `kzg_verify_multiproof_batch_locate`):
csrc/host_locate.h as a plain g++ program (tests/hostcheck/locatecheck.cpp states each check: the counting-sort plan against a naive
stable sort, the search over planted bad groups with its bound on predicate calls, the search with the real host pairing), built once
plainly and once with AddressSanitizer and UBSan; the declarations of the two entries; the argument errors that need no device."""
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
ENTRIES = ("kzg_coset_group_sums", "kzg_verify_multiproof_batch_locate")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_host_locate_as_a_host_program(tmp_path, flags):
    """A stand-alone binary with its own main, run directly (no preloaded runtime)."""
    exe = str(tmp_path / "locatecheck")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", *flags, "-I" + CSRC,
                           os.path.join(HERE, "hostcheck", "locatecheck.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "locatecheck ok", (r.stdout[-500:], r.stderr[-3000:])


def test_host_locate_header_includes_no_hip():
    src = open(os.path.join(CSRC, "host_locate.h")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert includes and not any("hip" in inc for inc in includes), includes
    assert "kzg_ctx" not in src.replace("no kzg_ctx", "")


def test_header_prototypes_and_exports_agree_on_the_two_entries():
    import rust_kzg_bn254_amd as k
    hdr = open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read()
    lib = C.CDLL(k._lib.LIB_PATH)
    L = k._lib
    for name in ENTRIES:
        decl = re.search(r"\bint32_t %s\s*\(([^;]*)\);" % name, hdr)
        assert decl, name
        assert name in L.PROTOTYPES and hasattr(lib, name), name
        assert len(decl.group(1).split(",")) == len(L.PROTOTYPES[name][1]), name
    batch = L.PROTOTYPES["kzg_verify_multiproof_batch"][1]
    szp = C.POINTER(L.sz)
    # the batch entry's arguments without g2_tau_l and out_ok, then the partition and the outputs
    assert L.PROTOTYPES["kzg_coset_group_sums"] == (L.i32, batch[:12] + [L.u64p, L.sz, L.u64p, L.u8p, L.u64p, L.u8p])
    assert L.PROTOTYPES["kzg_verify_multiproof_batch_locate"] == (L.i32, batch[:13] + [L.u64p, L.sz, L.u8p, szp, szp])
    params = [p.split()[-1].lstrip("*") for p in re.search(r"\bint32_t kzg_coset_group_sums\s*\(([^;]*)\);", hdr).group(1).split(",")]
    assert params[-6:] == ["group_indices", "n_groups", "out_lhs_xy_mont", "out_lhs_is_infinity", "out_rhs_xy_mont", "out_rhs_is_infinity"]
    assert "kzg_srs* srs" in re.search(r"\bint32_t kzg_coset_group_sums\s*\(([^;]*)\);", hdr).group(1).replace("const kzg_srs", "")


class _FakeSrs:
    handle = None

    def __len__(self):
        return 64


def test_argument_errors_that_need_no_device():
    """The null context is the first check of both entries, as it is of the batch entry: every call below returns before it needs a
    device, and writes no output.  The rest of the table needs a context and an SRS (tests/test_gpu_multiproof_locate.py).  The Python
    surface refuses its own argument errors without creating a context."""
    import rust_kzg_bn254_amd as k
    from rust_kzg_bn254_amd import verifier
    lib = k.load()
    L = k._lib
    one = pyref.frs_to_mont([1])
    pt = np.zeros((1, 8), np.uint64)
    idx = np.zeros(1, np.uint64)
    ys = np.zeros((1, 2, 4), np.uint64)
    g2 = k.helpers.g2_generator()
    out = np.full((1, 8), 7, np.uint64)
    flag = np.full(1, 7, np.uint8)
    bad, checks = L.sz(7), L.sz(7)
    u8 = lambda a: a.ctypes.data_as(L.u8p)                                      # noqa: E731
    P = L.ptr
    assert lib.kzg_coset_group_sums(None, None, P(pt), 1, P(idx), P(idx), P(ys), P(pt), 1, 8, 2, P(one), P(idx), 1, P(out), u8(flag), P(out),
                                    u8(flag)) == L.ERR_INVALID_ARG
    assert lib.kzg_coset_group_sums(None, None, None, 0, None, None, None, None, 0, 8, 2, None, None, 0, None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.kzg_verify_multiproof_batch_locate(None, None, P(pt), 1, P(idx), P(idx), P(ys), P(pt), 1, 8, 2, P(one), P(g2), P(idx), 1, u8(flag),
                                                  C.byref(bad), C.byref(checks)) == L.ERR_INVALID_ARG
    assert lib.kzg_verify_multiproof_batch_locate(None, None, P(pt), 1, P(idx), P(idx), P(ys), P(pt), 1, 8, 2, P(one), None, None, 0, None, None,
                                                  None) == L.ERR_INVALID_ARG
    assert (out == 7).all() and flag[0] == 7 and bad.value == 7 and checks.value == 7
    before = dict(L._default_ctx)                                               # device id -> Context: must not grow
    G = k.errors.GenericError
    with pytest.raises(G, match="tau\\^l"):
        verifier.locate_bad_multiproofs([pt[0]], [0], [0], ys, [pt[0]], 8, _FakeSrs(), g2_tau_l=None)
    with pytest.raises(G, match="not the same"):
        verifier.locate_bad_multiproofs([pt[0]], [0, 0], [0], ys, [pt[0]], 8, _FakeSrs(), g2_tau_l=g2)
    with pytest.raises(G, match="not the same"):
        verifier.locate_bad_multiproofs([pt[0]], [0], [0], ys, [pt[0]], 8, _FakeSrs(), g2_tau_l=g2, groups=[0, 0], n_groups=1)
    with pytest.raises(G, match="n_groups"):
        verifier.coset_group_sums([pt[0]], [0], [0], ys, [pt[0]], 8, _FakeSrs(), groups=[0])
    with pytest.raises(G, match="commitment"):
        verifier.coset_group_sums([pt[0]], [0], [0], ys, [pt[0]], 8, _FakeSrs(), groups="row")
    with pytest.raises(k.errors.InvalidInputLength):
        verifier.coset_group_sums([pt[0]], [0], [0], np.zeros((1, 8), np.uint64), [pt[0]], 8, _FakeSrs())
    assert L._default_ctx == before
