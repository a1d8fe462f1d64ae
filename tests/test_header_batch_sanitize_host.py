"""The new host code of batched header verification (the weight transcript of csrc/host_fiat_shamir.h, pairings_product_is_one of
csrc/host_pairing.h) in a stand-alone program under AddressSanitizer and UBSan: tests/hostcheck/header_batch_sanitize_main.cpp has its
own main and links nothing of the library.  No GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rust-kzg-bn254_amd", "csrc")


def test_weights_and_pairing_product_stand_alone_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "header_batch_sanitize_main")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                           "-I" + CSRC, os.path.join(HERE, "hostcheck", "header_batch_sanitize_main.cpp"), "-lpthread", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "header batch sanitize ok", (r.stdout[-500:], r.stderr[-3000:])
