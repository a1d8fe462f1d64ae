"""CPU: the MSM planner (csrc/msm_plan.h) and the host epilogue (csrc/host_msm_epilogue.h) as plain g++ programs, no GPU and no library.
The plan of every case of a fixed grid must equal tests/golden/msm_plans.txt -- recorded from the planner as it stood inside msm.hip
before it became a header (profiles/msm_driver.md), never from the code under test -- and satisfy the invariants plancheck.cpp states;
the epilogue of every MSM form must give (sum weight k) G for known bucket values."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rust-kzg-bn254_amd", "csrc")


def build(tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, os.path.join(HERE, "hostcheck", name + ".cpp"), "-o", exe])
    return exe


def test_plans_equal_the_recorded_table_and_keep_their_invariants(tmp_path):
    r = subprocess.run([build(tmp_path, "plancheck")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    want = open(os.path.join(HERE, "golden", "msm_plans.txt")).read().splitlines()
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d" % (i + 1)
    # the grid rejects something at every check the planner has, and accepts every mode
    assert sum(" status=-" in ln for ln in want) >= 9 and any(" error=" in ln for ln in want)
    for mode in (" bitsum=1", " fused=1", " naf=1", " sort2=1", " lean=1", " quad1=1", " quad1=0", " tables=0", " idx_log=20"):
        assert any(mode in ln for ln in want), mode


def test_host_epilogue_against_the_definition(tmp_path):
    r = subprocess.run([build(tmp_path, "epiloguecheck")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "epiloguecheck ok", (r.stdout[-500:], r.stderr[-3000:])
