"""CPU: the planner of the G2 MSM driver (csrc/g2msm_plan.h) as a plain g++ program, no GPU and no library: every n in 1 .. 2^20 that is a
power of two or one beside it, and every n at which the plan changes shape, gives a plan that passes its own status function; workspace
bytes are monotone within a shape; the accumulate lanes are those of the lane rule exactly; the buffers are as large as the kernels
index them (tests/hostcheck/g2msm_plan_grid.h states the invariants).  This module reads the program's lines of ONE blob (the single
call); tests/test_g2msm_batch_plan_host.py reads those of the groups.  The plans of the commit before single and batched calls shared
one planner are kept under tests/golden/: what the single call's plan kept of them, and that no batch plan moved, is asserted here."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rust-kzg-bn254_amd", "csrc")
WAVE_SLOTS = 2048


def fields(ln):
    return {k: int(v) for k, v in (f.split("=") for f in ln.split())}


@pytest.fixture(scope="module")
def stdout(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("g2p") / "g2msm_plancheck")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, os.path.join(HERE, "hostcheck", "g2msm_plancheck.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.splitlines()


def test_g2_plans_pass_their_status_and_keep_their_invariants(stdout):
    lines = [ln for ln in stdout if " count=" not in ln]
    ns = sorted({int(ln.split()[0][2:]) for ln in lines})
    for k in range(21):
        for n in (2 ** k - 1, 2 ** k, 2 ** k + 1):
            assert n in ns or n == 0 or n > 2 ** 20, n
    # the grid crosses every shape boundary: each window width from 4 to 14, both sort forms, both scan forms, free and saturated lanes
    cs = {int(ln.split()[2][2:]) for ln in lines}
    assert cs == set(range(4, 15))
    for field in (" small=0", " small=1", " scan1=0", " scan1=1", " nb=2"):
        assert any(field in ln for ln in lines), field
    # both sides of every window boundary below 4 097 are cases (tests/test_gpu_g2_msm.py runs them on the device)
    for n in (2047, 2048, 4095, 4096):
        assert n in ns


def test_the_single_plan_keeps_what_the_parent_planned_except_the_capped_lanes(stdout):
    new = {(r["n"], r["nb"]): r for r in map(fields, (ln for ln in stdout if " count=" not in ln))}
    old = [fields(ln) for ln in open(os.path.join(HERE, "golden", "g2_single_plans_parent.txt"))]
    assert len(old) == 124
    capped = 0
    for o in old:
        r = new[(o["n"], o["nb"])]
        for f in ("c", "W", "B", "T", "m", "small", "scan1", "n_out"):
            assert r[f] == o[f], (o["n"], o["nb"], f)
        E, G = o["W"] * o["n"], o["W"] * o["B"]
        if 4 * G < min(64 * WAVE_SLOTS, -(-E // 4)):                 # the bucket cap is the smallest term of the lane rule
            capped += 1
            assert r["nl"] == max(256, -(-4 * G // 256) * 256) <= o["nl"]
        else:
            assert (r["nl"], r["seg"]) == (o["nl"], o["seg"]), (o["n"], o["nb"])
        if o["nb"] == 1:
            assert r["launches"] == o["launches"], o["n"]
    assert 0 < capped < len(old)


def test_no_batch_plan_moved(stdout):
    want = [ln.rstrip("\n") for ln in open(os.path.join(HERE, "golden", "g2_batch_plans_parent.txt"))]
    assert len(want) == 210
    got = set(stdout)
    for ln in want:
        assert ln in got, ln
