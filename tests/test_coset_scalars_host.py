"""CPU: the host scalars of the coset-proof batch equation (csrc/host_coset_verify.h: r_i | r_i w^(k_i l) | the row sums of the weights, in the
order of the bases proofs | proofs | commitments) as a plain g++ program, no GPU and no library, against Python big integers.  The program
(tests/hostcheck/cosetscalarcheck.cpp) states its inputs; the cases: m = 2 (the high power table has one entry), an odd and an even log m, coset
index 0 and m - 1, N = 1, 1023, 1024, 1025 (the edge of the 32-chunk split), M > N (rows of weight zero), every item on one row.  The same
program is built once more with AddressSanitizer and UBSan as a stand-alone executable and must print the same lines."""
import os
import subprocess

import pytest

import pyref

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rust-kzg-bn254_amd", "csrc")
R = pyref.R_
MASK = (1 << 64) - 1
CASES = [(1, 1, 1, 2, 1), (1, 1025, 3, 2, 1), (5, 1023, 4, 2, 1), (6, 1024, 4, 2, 1), (6, 1025, 2000, 2, 1), (5, 7, 12, 0, 1), (5, 7, 3, 1, 0),
         (6, 1, 5, 1, 0), (23, 1030, 2, 2, 1)]


def wire(v):
    return v % R * pyref.MONT_R % R


def expected(log_m, N, M, kmode, cmode):
    m = 1 << log_m
    w = pyref.root_of_unity(log_m)
    rs, shifted, rows = [], [], [0] * M
    for i in range(N):
        a = (i + 1) * 0x9e3779b97f4a7c15 & MASK
        x = a | (~a & MASK) << 64 | (3 * a & MASK) << 128 | (i & 0xffff) << 192
        k = 0 if kmode == 0 else m - 1 if kmode == 1 else (0, m - 1, (2654435761 * i + 3) % m)[i % 3]
        c = M - 1 if cmode == 0 else i % M
        rs.append(wire(x))
        shifted.append(wire(x * pow(w, k, R)))
        rows[c] = (rows[c] + x) % R
    return rs + shifted + [wire(v) for v in rows]


def build_and_run(tmp, flags):
    exe = str(tmp / "cosetscalarcheck")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", *flags, "-I" + CSRC,
                           os.path.join(HERE, "hostcheck", "cosetscalarcheck.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    return build_and_run(tmp_path_factory.mktemp("cosetscalars"), ["-O2"])


@pytest.fixture(scope="module")
def scalars(output):
    out = {}
    for ln in output.splitlines():
        f = ln.split()
        out[tuple(int(v) for v in f[:5])] = [int(v, 16) for v in f[5:]]
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "logm%d-N%d-M%d-k%d-c%d" % c)
def test_scalars_equal_big_integers(scalars, case):
    log_m, N, M, kmode, cmode = case
    got, want = scalars[case], expected(*case)
    assert len(got) == 2 * N + M
    assert got[:N] == want[:N], "the weights"
    assert got[N:2 * N] == want[N:2 * N], "the shifted weights"
    assert got[2 * N:] == want[2 * N:], "the row sums"
    if M > N and cmode == 1:
        assert got[2 * N + N:] == [0] * (M - N), "rows without an item"
    if cmode == 0:
        assert got[2 * N:-1] == [0] * (M - 1), "every item on the last row"


def test_every_case_was_printed(scalars):
    assert sorted(scalars) == sorted(CASES)


def test_same_lines_under_address_and_ub_sanitizers(tmp_path, output):
    """A stand-alone binary with its own main, run directly (no preloaded runtime)."""
    assert build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]) == output


def test_header_includes_no_hip():
    src = open(os.path.join(CSRC, "host_coset_verify.h")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert includes and not any("hip" in inc or "engine" in inc for inc in includes), includes
