"""-m gpu: `KZG::encode_cosets` of the C++ mirror (include/kzg_bn254_mi355x.hpp).  tests/cpp/encode_mirror.cpp encodes 64 coefficients on
256 points over a known-tau SRS of 64 points in its own process (no Python on the product side), checks the evaluation form, each output
alone and the errors of the method, and prints values and proofs; this file builds and runs it and compares them, bit for bit, with the
Python mirror."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import pyref
from pyref import R_

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/encode/v1").digest(), "big") % R_


def test_cpp_encode_cosets_equals_the_python_mirror(tmp_path):
    import rust_kzg_bn254_amd as k
    exe = str(tmp_path / "encode_mirror")
    libdir = os.path.join(ROOT, "rust-kzg-bn254_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "encode_mirror.cpp"), "-L" + libdir, "-lkzg_bn254_mi355x", "-Wl,-rpath," + libdir, "-o", exe])
    res = subprocess.run([exe, "%064x" % TAU], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.splitlines()[-1] == "encode_mirror ok", (res.returncode, res.stdout[-500:], res.stderr[-1500:])
    vals = {ln.split()[0]: ln.split()[1] for ln in res.stdout.splitlines() if " " in ln}
    d, n, l = 64, 256, 4
    srs = k.SRS.generate(TAU, d)
    ys, proofs = k.KZG.new().encode_cosets(k.PolynomialCoeffForm(pyref.frs_to_mont([(i + 3) ** 2 for i in range(d)])), srs, n, l)
    srs.close()
    assert vals["ys"] == "".join("%016x" % int(w) for w in ys.reshape(-1))
    assert vals["proofs"] == "".join("%016x" % int(w) for w in np.asarray(proofs).reshape(-1))
