"""CPU: the host side of `kzg_encode_cosets` (csrc/host_encode.h) as a plain g++ program built with AddressSanitizer and UBSan and run
on its own, no GPU and no library: the error table in its documented order, the sizes and workspace bytes of fixed shapes, and the plan
of the zero-padded G1 transform -- the spread factor, the stage range of the radix-2 form, the grids, and r = 1 being the plan of
g1_fft_planes (tests/hostcheck/encodecheck.cpp states each check)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rust-kzg-bn254_amd", "csrc")


def test_encode_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "encodecheck")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(HERE, "hostcheck", "encodecheck.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "encodecheck ok", (r.stdout[-500:], r.stderr[-3000:])


def test_host_encode_header_includes_no_hip():
    src = open(os.path.join(CSRC, "host_encode.h")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert includes and not any("hip" in inc for inc in includes), includes
    plan = open(os.path.join(CSRC, "g1fft_plan.h")).read()           # the header it builds on is host code too
    assert not any("hip" in ln for ln in plan.splitlines() if ln.startswith("#include"))
