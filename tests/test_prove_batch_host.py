"""No GPU: the host-checkable half of the batched prover (`kzg_compute_proof_batch`, `kzg_compute_blob_proof_batch`,
`kzg_commit_and_prove_blob_batch`).

  1. The lane functions of the fused evaluate-and-divide kernel (csrc/provebatch_lanes.h) built for the host with the bound-checked field
     (tests/hostcheck/provebatchcheck.cpp, g++ -DKZG_BOUND_CHECK) and run as one workgroup lane by lane at n = 2, 64, 512, 1 024, 2 048 and
     4 096 (every lanes-per-element instantiation): random z, z = w^0, w^(n-1), w^(n/2), z = 0, against rows that are random, all zero,
     constant and all r - 1.  y and every q_j are big-integer values computed here over tests/pyref.py's field; at n = 2 and 64 those values
     are first checked against the polynomial itself (coefficients by pyref.dft, synthetic division by X - z).  No bound-check report on
     stderr; the on-domain root inverse z / n is checked against the product it replaces inside the program.
  2. The planner (csrc/host_prove_batch.h) through a stand-alone program (tests/hostcheck/provebatchplancheck.cpp), plain and under
     ASan + UBSan: the error order row by row, mixed lengths, groups of one, a blob over 2^12 elements, count = 0, the scatter a permutation.
  3. The ABI surface: parameter names against the header, the `_lib.py` table, the error rows that need no device.
"""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

import pyref

R_ = pyref.R_
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
LANES_SRC = os.path.join(HERE, "hostcheck", "provebatchcheck.cpp")
PLAN_SRC = os.path.join(HERE, "hostcheck", "provebatchplancheck.cpp")
SIZES = (2, 64, 512, 1024, 2048, 4096)


def _build(src, exe, extra):
    subprocess.check_call(["g++", "-std=c++17", "-DKZG_BOUND_CHECK", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", *extra, "-I" + CSRC, src, "-o", exe])


# ---- big integers ------------------------------------------------------------------------------------------------------------------------------
def reference(f, z, n, w):
    """(on_domain, m, y, q) of KZG::compute_proof's quotient (kzg.rs:151-174, :237-260; helpers.rs:485-532) in plain modular arithmetic."""
    roots = [pow(w, j, R_) for j in range(n)]
    if pow(z, n, R_) == 1:
        m = roots.index(z)
        y = f[m]
        q = [0] * n
        for j in range(n):
            if j != m:
                q[j] = (f[j] - y) * pow(roots[j] - z, -1, R_) % R_
        # kzg.rs:237-260: sum over i != m of (f_i - y) w^i / ((z - w^i) z)
        q[m] = sum((f[j] - y) * roots[j] % R_ * pow((z - roots[j]) * z, -1, R_) for j in range(n) if j != m) % R_
        return True, m, y, q
    total = sum(f[j] * roots[j] % R_ * pow(z - roots[j], -1, R_) for j in range(n)) % R_
    y = (pow(z, n, R_) - 1) * pow(n, -1, R_) % R_ * total % R_
    return False, 0, y, [(f[j] - y) * pow(roots[j] - z, -1, R_) % R_ for j in range(n)]


def by_division(f, z, n):
    """The same from the polynomial: coefficients, y = f(z), (f - y) / (X - z) by synthetic division, its values on the domain."""
    coeffs = pyref.dft(f, inverse=True)
    y = pyref.poly_eval(coeffs, z)
    quo, carry = [0] * n, 0
    for k in range(n - 1, 0, -1):
        carry = (coeffs[k] + carry * z) % R_
        quo[k - 1] = carry
    assert (coeffs[0] + carry * z) % R_ == y
    return y, pyref.dft(quo)


def cases(n, seed):
    rnd = random.Random(seed)
    w = pyref.root_of_unity(n.bit_length() - 1)
    c = rnd.randrange(1, R_)
    rows = [[rnd.randrange(R_) for _ in range(n)], [0] * n, [c] * n, [R_ - 1] * n]
    zs = [rnd.randrange(R_), 1, pow(w, n - 1, R_), pow(w, n // 2, R_), 0]
    return w, [(f, z) for f in rows for z in zs]


def words(v):
    return struct.pack("<8I", *[(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)])


def wire(v):
    return words(v % R_ * pyref.MONT_R % R_)


def case_file(n, seed):
    log_n = n.bit_length() - 1
    w, cs = cases(n, seed)
    w4096 = pyref.root_of_unity(12)
    internal = 1 << 261
    out = [struct.pack("<2I", log_n, len(cs))]
    out += [words(pow(w4096, i, R_) * internal % R_) for i in range(64)]
    out += [words(pow(w4096, 64 * i, R_) * internal % R_) for i in range(64)]
    on = 0
    for f, z in cs:
        od, m, y, q = reference(f, z, n, w)
        on += od
        out.append(struct.pack("<2I", int(od), m))
        out.append(wire(z))
        out += [wire(v) for v in f]
        out.append(wire(y))
        out += [wire(v) for v in q]
    return b"".join(out), len(cs), on


@pytest.mark.parametrize("n", [2, 64])
def test_the_reference_values_are_the_polynomials_quotient(n):
    w, cs = cases(n, 1000 + n)
    for f, z in cs:
        od, m, y, q = reference(f, z, n, w)
        y2, q2 = by_division(f, z, n)
        assert od == (pow(z, n, R_) == 1) and y == y2 and q == q2
        if od:
            assert pow(w, m, R_) == z
    assert sum(pow(z, n, R_) == 1 for _, z in cs) >= 8                                 # the domain points are among the cases


@pytest.fixture(scope="module")
def lanes_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("provebatch") / "provebatchcheck")
    _build(LANES_SRC, exe, ["-O1"])
    return exe


@pytest.mark.parametrize("n", SIZES)
def test_lane_functions_lane_by_lane_against_big_integers(lanes_exe, tmp_path, n):
    data, count, on = case_file(n, 1000 + n)
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        fh.write(data)
    r = subprocess.run([lanes_exe, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "KZG_BOUND_CHECK" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.strip() == "prove batch ok log_n=%d cases=%d on_domain=%d" % (n.bit_length() - 1, count, on)
    assert count == 20 and on == 12                                                    # three domain points against each of the four rows


def test_lane_functions_stand_alone_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "provebatchcheck_san")
    _build(LANES_SRC, exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for n in (2, 64, 1024):
        data, count, on = case_file(n, 2000 + n)
        path = str(tmp_path / ("cases%d.bin" % n))
        with open(path, "wb") as fh:
            fh.write(data)
        r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0 and "KZG_BOUND_CHECK" not in r.stderr, (r.stdout[-500:], r.stderr[-3000:])
        assert r.stdout.strip() == "prove batch ok log_n=%d cases=%d on_domain=%d" % (n.bit_length() - 1, count, on)


# ---- the planner ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_planner_stand_alone(tmp_path, extra):
    exe = str(tmp_path / "provebatchplancheck")
    _build(PLAN_SRC, exe, extra)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.strip() == "prove batch plan ok" and r.stderr == ""


# ---- the ABI surface (the library loads without a GPU) -------------------------------------------------------------------------------------
ENTRIES = {
    "kzg_compute_proof_batch": ["ctx", "srs", "evals_mont", "n", "count", "zs_mont", "out_proofs_xy_mont", "out_is_infinity", "out_ys_mont"],
    "kzg_compute_proof_batch_device": ["ctx", "srs", "d_evals_mont", "n", "count", "zs_mont", "out_proofs_xy_mont", "out_is_infinity", "out_ys_mont"],
    "kzg_compute_blob_proof_batch": ["ctx", "srs", "blobs", "blob_lens", "commitments_xy_mont", "count", "out_proofs_xy_mont", "out_is_infinity", "out_zs_mont",
                                     "out_ys_mont", "out_bad_index"],
    "kzg_commit_and_prove_blob_batch": ["ctx", "srs", "blobs", "blob_lens", "count", "out_commitments_xy_mont", "out_commitment_is_infinity", "out_proofs_xy_mont",
                                        "out_proof_is_infinity", "out_zs_mont", "out_ys_mont", "out_bad_index"],
    "kzg_ctx_set_prove_group_bytes": ["ctx", "bytes"],
}


def test_the_c_abi_declares_the_entries_with_these_parameters():
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read(), flags=re.S)
    from rust_kzg_bn254_amd import _lib
    lib = _lib.load()
    for name, params in ENTRIES.items():
        decl = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert decl, name
        names = [re.sub(r"\[.*\]", "", p).split()[-1].lstrip("*") for p in decl.group(1).split(",")]
        assert names == params, (name, names)
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == len(params) and hasattr(lib, name)
    assert "n_roots" not in re.search(r"int32_t\s+kzg_compute_proof_batch\s*\(([^)]*)\)", header).group(1)
    import rust_kzg_bn254_amd as k
    assert callable(k.KZG.compute_proof_batch) and callable(k.KZG.compute_blob_proof_batch) and callable(k.KZG.commit_and_prove_blob_batch)
    assert callable(k.Context.set_prove_group_bytes)


def test_the_error_rows_that_need_no_device():
    from rust_kzg_bn254_amd import _lib as L
    lib = L.load()
    z = np.zeros(64, dtype=np.uint64)
    zb = z.ctypes.data_as(L.u8p)
    ptrs = (C.c_char_p * 1)(b"\x00" * 32)
    lens = (L.sz * 1)(32)
    bad = C.c_size_t(7)
    # null handles, whatever else is wrong (no handle is dereferenced) -- in front of count = 0
    assert lib.kzg_compute_proof_batch(None, None, L.ptr(z), 4, 1, L.ptr(z), L.ptr(z), zb, L.ptr(z)) == L.ERR_INVALID_ARG
    assert lib.kzg_compute_proof_batch(None, None, None, 3, 0, None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.kzg_compute_proof_batch_device(None, None, None, 4, 0, None, L.ptr(z), None, None) == L.ERR_INVALID_ARG
    assert lib.kzg_compute_blob_proof_batch(None, None, ptrs, lens, L.ptr(z), 1, L.ptr(z), zb, L.ptr(z), L.ptr(z), C.byref(bad)) == L.ERR_INVALID_ARG
    assert lib.kzg_compute_blob_proof_batch(None, None, None, None, None, 0, None, None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.kzg_commit_and_prove_blob_batch(None, None, ptrs, lens, 1, L.ptr(z), zb, L.ptr(z), zb, L.ptr(z), L.ptr(z), C.byref(bad)) == L.ERR_INVALID_ARG
    assert lib.kzg_commit_and_prove_blob_batch(None, None, None, None, 0, None, None, None, None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.kzg_ctx_set_prove_group_bytes(None, 1) == L.ERR_INVALID_ARG
    assert bad.value == 7
    # the Python surface refuses shapes before it looks for a device
    import rust_kzg_bn254_amd as k

    class FakeSrs:
        handle = None

        def __len__(self):
            return 16

    kz = k.KZG.__new__(k.KZG)
    one = np.zeros(4, dtype=np.uint64)
    with pytest.raises(k.errors.GenericError, match="one length"):
        kz.compute_proof_batch([np.zeros((4, 4), np.uint64), np.zeros((8, 4), np.uint64)], [one, one], FakeSrs())
    with pytest.raises(k.errors.GenericError, match="one point per polynomial"):
        kz.compute_proof_batch([np.zeros((4, 4), np.uint64)], [one, one], FakeSrs())
    with pytest.raises(k.errors.GenericError, match="array"):
        kz.compute_proof_batch(np.zeros((4, 4), np.uint64), [one], FakeSrs())
    with pytest.raises(k.errors.SrsCapacityExceeded):
        kz.compute_proof_batch(np.zeros((2, 32, 4), np.uint64), [one, one], FakeSrs())
    out, y = kz.compute_proof_batch([], [], FakeSrs(), want_y=True)                    # count = 0: nothing to do, no device
    assert out.shape == (0, 8) and y.shape == (0, 4)
