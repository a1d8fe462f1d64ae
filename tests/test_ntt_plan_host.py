"""CPU: the Fr NTT planner (csrc/ntt_plan.h) as a plain g++ program, no GPU and no library.  The plan of every case of a fixed grid -- every log n
from 1 to 28, both directions, no tile override / 10 / 11, 256 and 8 CUs, the per-element twiddle arrays granted or refused -- must equal
tests/golden/ntt_plans.txt, recorded from ntt_run as it stood inside ntt.hip before the planner became a header (profiles/scalar_drivers.md), never
from the code under test, and satisfy the invariants ntt_plancheck.cpp states.  The file writes a plan once and names it by its number
(tests/hostcheck/ntt_grid.h)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rust-kzg-bn254_amd", "csrc")


def test_plans_equal_the_recorded_table_and_keep_their_invariants(tmp_path):
    exe = str(tmp_path / "ntt_plancheck")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + CSRC, os.path.join(HERE, "hostcheck", "ntt_plancheck.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    want = open(os.path.join(HERE, "golden", "ntt_plans.txt")).read().splitlines()
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d" % (i + 1)
    # every case of the grid is there: 28 sizes x 2 directions, each line naming 3 tile settings x 2 CU counts x arrays granted / refused
    groups = [ln.split(" -> ")[1].split() for ln in want if ln.startswith("ntt ")]
    assert len(groups) == 28 * 2 and all(len(g) == 12 for g in groups)
    plans = [ln for ln in want if ln.startswith("#")]
    assert {int(tok.split("=#")[1]) for g in groups for tok in g} == set(range(len(plans)))
    # the grid reaches every instantiation, one to three passes, both arms of min(tiles, CUs x k), every buffer, and the refused fold
    for kernel in ("k_ntt_pass<11,10>", "k_ntt_pass<10,10>", "k_ntt_pass<10,7>", "k_ntt_pass<10,8>", "k_ntt_pass<10,9>"):
        assert any(" %s " % kernel in ln for ln in plans), kernel
    for passes in (1, 2, 3):
        assert any(" passes=%d " % passes in ln for ln in plans), passes
    pass_lines = [part.split() for ln in plans for part in ln.split(" | ")[1:]]
    field = lambda ln, key: next(f[len(key) + 1:] for f in ln if f.startswith(key + "="))
    assert any(field(ln, "grid") == field(ln, "tiles") for ln in pass_lines) and any(int(field(ln, "grid")) < int(field(ln, "tiles")) for ln in pass_lines)
    for route in ("caller->caller", "caller->data", "data->caller", "data->tmp", "tmp->caller"):
        assert any(route in ln for ln in pass_lines), route
    for tw in ("-", "plain:given", "plain:refused", "scaled:given", "scaled:refused"):
        assert any(field(ln, "tw") == tw for ln in pass_lines), tw
    # a refused scaled array leaves the 1 / n in the last pass: the pass behind a boundary whose fold was refused scales itself
    refused = [ln.split(" | ") for ln in plans if "tw=scaled:refused" in ln]
    assert refused and all("next=0/0 " in ln[-1] and "scale=-1" not in ln[-1] and "tw=scaled:refused" in ln[-2] for ln in refused)
    given = [ln.split(" | ") for ln in plans if "tw=scaled:given" in ln]
    assert given and all("scale=-1" in ln[-1] for ln in given)
