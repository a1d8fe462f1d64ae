"""CPU: the G1 FFT planner (csrc/g1fft_plan.h) as a plain g++ program, no GPU and no library.  The plan of every case of a fixed grid -- every
log n from 0 to 24 on every SRS shape for g1_ifft, every log n from 0 to 20 in every direction for the planes transform -- must equal
tests/golden/g1fft_plans.txt, recorded from the driver as it stood inside g1fft.hip before the planner became a header
(profiles/g1fft_driver.md), never from the code under test, and satisfy the invariants g1fft_plancheck.cpp states.  The file names a plan that an earlier case already had
by its number only (tests/hostcheck/g1fft_grid.h)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rust-kzg-bn254_amd", "csrc")


def test_plans_equal_the_recorded_table_and_keep_their_invariants(tmp_path):
    exe = str(tmp_path / "g1fft_plancheck")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + CSRC, os.path.join(HERE, "hostcheck", "g1fft_plancheck.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    want = open(os.path.join(HERE, "golden", "g1fft_plans.txt")).read().splitlines()
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d" % (i + 1)
    # every case of the grid is there: 13 SRS shapes x 25 sizes + 11 sizes of the short SRS, 21 sizes x 8 directions of the planes transform
    assert sum(ln.startswith("ifft ") for ln in want) == 13 * 25 + 11 and sum(ln.startswith("planes ") for ln in want) == 21 * 8
    # the grid reaches every form and every stage kind (load and gather each plain and bit-reversed), from both drivers
    for form in ("copy", "bits", "bits+quads", "tables+direct", "direct", "radix2"):
        assert any(" form=%s " % form in ln for ln in want), form
        if form in ("copy", "direct", "radix2"):
            assert any(ln.startswith("planes ") and " form=%s " % form in ln for ln in want), form
    stage_lines = [ln for ln in want if ln.startswith("    ")]
    for kernel in ("k_g1fft_load", "k_g1fft_gather_planes", "k_g1fft_bits", "k_g1fft_first_tables", "k_g1fft_direct", "k_g1fft_direct_pairs", "k_g1fft_mul_quads",
                   "k_g1fft_stage", "k_g1fft_stage_pairs"):
        assert any(ln.split()[0] == kernel for ln in stage_lines), kernel
    for kernel in ("k_g1fft_load", "k_g1fft_gather_planes"):
        for bitrev in (True, False):
            assert any(ln.split()[0] == kernel and (" bitrev=" in ln) == bitrev for ln in stage_lines), (kernel, bitrev)
    assert any(" tab=small " in ln for ln in want) and any(" tab=points " in ln for ln in want) and any(" t3_points=1024" in ln for ln in want)
    assert any(" in->tmp" in ln for ln in stage_lines) and any(" in->out" in ln for ln in stage_lines)
