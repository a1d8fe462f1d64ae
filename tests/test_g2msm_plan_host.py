"""CPU: the planner of the G2 MSM driver (csrc/g2msm_plan.h) as a plain g++ program, no GPU and no library: every n in 1 .. 2^20 that is a
power of two or one beside it, and every n at which the plan changes shape, gives a plan that passes its own status function; workspace
bytes are monotone within a shape; entries per accumulate lane stay within the stated bound; the buffers are as large as the kernels
index them (tests/hostcheck/g2msm_plan_grid.h states the invariants)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rust-kzg-bn254_amd", "csrc")


def test_g2_plans_pass_their_status_and_keep_their_invariants(tmp_path):
    exe = str(tmp_path / "g2msm_plancheck")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, os.path.join(HERE, "hostcheck", "g2msm_plancheck.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
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
