"""CPU: the host side of `kzg_recover_from_cosets` (csrc/host_recover.h) as a plain g++ program built with AddressSanitizer and
UBSan and run on its own, no GPU and no library: the error table in its documented order, the missing-coset list and item map, and the
cost cap at its edge (tests/hostcheck/recovercheck.cpp states each check)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rust-kzg-bn254_amd", "csrc")


def test_recover_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "recovercheck")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(HERE, "hostcheck", "recovercheck.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "recovercheck ok", (r.stdout[-500:], r.stderr[-3000:])


def test_host_recover_header_includes_no_hip():
    src = open(os.path.join(CSRC, "host_recover.h")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert includes and not any("hip" in inc for inc in includes), includes
