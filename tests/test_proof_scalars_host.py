"""CPU: the scalar table of a proof's inversion chain (csrc/proof_plan.h proof_fill_scalars) as a plain g++ program, no GPU and no library, against
Python big integers: zt[a] = z^(2^a), zt[log n + 1] = 1 / (1 - z^n) or zero when z is on the domain, then z^-(2^a) (zero off the domain) and the
three constants 1/(i - 1), -1/2, 1/(-i - 1); all in wire form (times 2^256).  At z = 1 the table must equal, word for word, the vector the driver
used to build by hand for the known-index form's table before proof_fill_scalars existed (profiles/scalar_drivers.md)."""
import os
import subprocess

import pytest

import pyref

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rust-kzg-bn254_amd", "csrc")
R = pyref.R_
LOGS = (0, 1, 9, 12, 20, 28)


def wire(v):
    return v % R * pyref.MONT_R % R


def constants():
    i = pow(5, (R - 1) // 4, R)
    return [wire(pow(i - 1, -1, R)), wire(pow(-2, -1, R)), wire(pow(-i - 1, -1, R))]


def expected(z, log_n):
    n = 1 << log_n
    on = pow(z, n, R) == 1
    pows = [wire(pow(z, 1 << a, R)) for a in range(log_n + 1)]
    top = 0 if on else wire(pow(1 - pow(z, n, R), -1, R))
    inv = [wire(pow(z, -(1 << a), R)) if on else 0 for a in range(log_n + 1)]
    return on, pows + [top] + inv + constants()


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("proof_scalars") / "proof_scalars")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + CSRC, os.path.join(HERE, "hostcheck", "proof_scalars.cpp"), "-o", exe])
    out = {}
    for ln in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=600).stdout.splitlines():
        f = ln.split()
        out[(int(f[0]), f[1])] = (f[2] == "1", [int(w, 16) for w in f[3:]])
    return out


@pytest.mark.parametrize("log_n", LOGS)
def test_table_equals_big_integers(tables, log_n):
    n = 1 << log_n
    w = pyref.root_of_unity(log_n) if log_n else 1
    for name, z, on_domain in (("off", 7, False), ("one", 1, True), ("w", w, True), ("w^(n-1)", pow(w, n - 1, R), True), ("zero", 0, False)):
        on, got = tables[(log_n, name)]
        want_on, want = expected(z, log_n)
        assert want_on == on_domain and on == on_domain, name
        assert len(got) == 2 * log_n + 6 and got == want, name


@pytest.mark.parametrize("log_n", LOGS)
def test_zero_gives_what_the_driver_gave_before(tables, log_n):
    """z = 0, recorded from the block inside proof_enqueue before it became a function: every power zero, 1 / (1 - 0) = 1, off the domain."""
    on, got = tables[(log_n, "zero")]
    assert not on and got == [0] * (log_n + 1) + [wire(1)] + [0] * (log_n + 1) + constants()


@pytest.mark.parametrize("log_n", range(1, 13))
def test_table_at_one_equals_the_hand_built_vector(tables, log_n):
    """the vector the known-index path filled by hand: one at zt[a] and zt[log n + 2 + a] for a <= log n, the constants at 2 log n + 3, zero elsewhere"""
    z1 = [0] * (2 * log_n + 6)
    for a in range(log_n + 1):
        z1[a] = z1[log_n + 2 + a] = wire(1)
    z1[2 * log_n + 3:] = constants()
    on, got = tables[(log_n, "z1")]
    assert on and got == z1
