"""CPU: the proof planner (csrc/proof_plan.h) as a plain g++ program, no GPU and no library.  The plan of every case of a fixed grid -- every log n
from 0 to 28, proof or evaluation only, with or without the inverse NTT, z off the domain / on it with its index found / on it without, the
evaluations on the host / already in the slot's buffer / resident in the caller's -- must equal tests/golden/proof_plans.txt, recorded from
proof_enqueue as it stood inside poly.hip before the planner became a header (profiles/scalar_drivers.md), never from the code under test, and
satisfy the invariants proof_plancheck.cpp states.  The file writes each part of a plan once and names it by its number
(tests/hostcheck/proof_grid.h)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rust-kzg-bn254_amd", "csrc")


def test_plans_equal_the_recorded_table_and_keep_their_invariants(tmp_path):
    exe = str(tmp_path / "proof_plancheck")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + CSRC, os.path.join(HERE, "hostcheck", "proof_plancheck.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    want = open(os.path.join(HERE, "golden", "proof_plans.txt")).read().splitlines()
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d" % (i + 1)
    # every case of the grid is there: 29 sizes x proof / evaluation x inverse NTT or not, each line naming 3 places of z x 3 sources
    groups = [[tok for tok in ln.split(" -> ")[1].split() if not tok.endswith(":")] for ln in want if ln.startswith("proof ")]
    assert len(groups) == 29 * 2 * 2 and all(len(g) == 9 for g in groups)
    chains = [ln for ln in want if ln.startswith("C")]
    tails = [ln for ln in want if ln.startswith("T")]
    used = [tok.split(",")[0].split("+") for g in groups for tok in g]
    assert {int(c[1:]) for c, _ in used} == set(range(len(chains))) and {int(t[1:]) for _, t in used} == set(range(len(tails)))
    assert sum(ln.startswith("size ") for ln in want) == 29
    # the grid reaches every form, every kernel and every other step, both streams, and builds the known-index table once per size
    for form in ("table", "small", "levels"):
        assert any(" form=%s " % form in ln for ln in chains), form
    steps = [step.split() for ln in chains + tails for step in ln.split("; ")[1:]]
    for step in ("k_poly_inv_small", "k_poly_inv_level", "k_poly_inverses", "k_poly_finish_y", "k_poly_quotient", "k_poly_quotient_on_domain", "k_poly_quotient_table",
                 "k_poly_quotient_on_domain_known", "upload_scalars", "upload_evals", "read_y", "intt", "record", "join", "check", "build"):
        assert any(ln[0] == step for ln in steps), step
    for step in ("upload_scalars", "k_poly_inv_small", "k_poly_inv_level"):
        for stream in ("main", "aux"):
            assert any(ln[0] == step and ln[1] == stream for ln in steps), (step, stream)
    assert sum(ln[0] == "build" for ln in steps) == 12
    text = "\n".join(want)
    assert " fused_y=1" in text and " fused_y=0" in text and " out=inv" in text and " out=lvl+" in text and ",a=0" in text and "tables=fi" in text
