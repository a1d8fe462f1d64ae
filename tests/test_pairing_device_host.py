"""Host-only (no GPU): the device pairing's headers on the CPU, and the surface of the batched pairing entries.
tests/hostcheck/pairingdevcheck.cpp compiles csrc/fq12.h, csrc/pairing_dev.h and csrc/host_pairing_batch.h with g++ and -DKZG_BOUND_CHECK (every
lazy-reduction bound is an abort) and compares BY VALUE with csrc/host_pairing.h: Fq12 product, square, line product, the three Frobenius
maps, conjugation, cyclotomic square, inverse and power by x on random operands and on the extreme limb patterns of tests/fe_operands.py; both
line steps along a whole loop; Miller products and checks of 0, 1, 2, 4, 5 and 6 pairs; bilinearity; the EIP-197 known answer of
tests/test_pairing_host.py; the constant tables; the argument table and the plan.  A stand-alone program with its own main: it runs once as
it is and once under AddressSanitizer + UndefinedBehaviorSanitizer, as a subprocess; nothing is loaded into Python under a sanitizer.  Plus
the ABI surface of the four new entries and their errors that need no device."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np

import fe_operands as fo
import pyref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
SRC = os.path.join(HERE, "hostcheck", "pairingdevcheck.cpp")
NAMES = ("kzg_pairings_product_verify_batch", "kzg_pairings_product_gt_batch", "kzg_pairings_product_gt", "kzg_ctx_set_locate_pairings")

# EIP-197, go-ethereum's bn256Pairing vector "jeff1" (tests/test_pairing_host.py checks every coordinate against its curve): two pairs, product one
EIP197 = """1c76476f4def4bb94541d57ebba1193381ffa7aa76ada664dd31c16024c43f59 3034dd2920f673e204fee2811c678745fc819b55d3e9d294e45c9b03a76aef41
            209dd15ebff5d46c4bd888e51a93cf99a7329636c63514396b4a452003a35bf7 04bf11ca01483bfa8b34b43561848d28905960114c8ac04049af4b6315a41678
            2bb8324af6cfc93537a2ad1a445cfd0ca2a71acd7ac41fadbf933c2a51be344d 120a2a4cf30c1bf9845f20c6fe39e07ea2cce61f0c9bb048165fe5e4de877550
            111e129f1cf1097710d41c4ac70fcdfa5ba2023c6ff1cbeac322de49d1b6df7c 2032c61a830e3c17286de9462bf242fca2883585b93870a73853face6a6bf411
            198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2 1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed
            090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b 12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa""".split()


def eip197_pairs():
    """(g1s (2, 8), g2s (2, 16)) wire words: EIP-197 writes an Fq2 element imaginary part first, the wire format is c0 | c1"""
    v = [int(h, 16) for h in EIP197]
    m = pyref.fq_to_mont
    g1s = [np.concatenate([m(v[0]), m(v[1])]), np.concatenate([m(v[6]), m(v[7])])]
    g2s = [np.concatenate([m(v[3]), m(v[2]), m(v[5]), m(v[4])]), np.concatenate([m(v[9]), m(v[8]), m(v[11]), m(v[10])])]
    return np.stack(g1s).astype(np.uint64), np.stack(g2s).astype(np.uint64)


def _operands(path):
    """the extreme signed limb patterns and the canonical edges, 9 int32 limbs each"""
    rnd = random.Random(41)
    rows = fo.extreme_patterns(rnd) + [fo.limbs(v) for v in fo.canonical_edges(pyref.P)]
    np.array(rows, dtype=np.int32).tofile(path)
    return len(rows)


def _build_and_run(tmp_path, exe, extra, env=None):
    ops = str(tmp_path / "operands.i32")
    assert _operands(ops) >= 60
    g1s, g2s = eip197_pairs()
    words = " ".join("%x" % int(w) for k in range(2) for w in list(g1s[k]) + list(g2s[k]))
    subprocess.check_call(["g++", "-std=c++17", "-DKZG_BOUND_CHECK", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", *extra, "-I" + CSRC, SRC, "-o", exe])
    r = subprocess.run([exe, ops, words], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "pairingdevcheck ok", (r.stdout[-500:], r.stderr[-3000:])


def test_device_pairing_headers_against_the_host_pairing(tmp_path):
    _build_and_run(tmp_path, str(tmp_path / "pairingdevcheck"), ["-O1"])


def test_the_same_program_under_asan_ubsan(tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    _build_and_run(tmp_path, str(tmp_path / "pairingdevcheck_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"],
                   env)


def test_the_new_exports_exist_with_their_declared_signatures():
    import rust_kzg_bn254_amd as k
    L = k._lib
    lib = L.load()                                                     # loading needs no GPU
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read(), flags=re.S)
    ctype = {"kzg_ctx*": L.vp, "const uint64_t*": L.u64p, "uint64_t*": L.u64p, "uint8_t*": L.u8p, "size_t": L.sz, "int32_t": L.i32}
    for name in NAMES:
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name + " is not declared in the header"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        types = [re.sub(r"\s*\w+$", "", p).replace(" *", "*") for p in params]      # drop the parameter's name
        res, args = L.PROTOTYPES[name]
        want = [ctype[t] for t in types]
        assert res is L.i32 and len(want) == len(args), (name, types)
        for w, a in zip(want, args):                                   # (pointer types are compared by what they point to)
            assert w is a or (hasattr(w, "_type_") and hasattr(a, "_type_") and w._type_ is a._type_), (name, types)
        assert hasattr(lib, name), name + " is not exported"
    for f in ("pairings_product_verify_batch", "pairings_product_gt_batch", "pairings_product_gt"):
        assert hasattr(k.verifier, f), f
    assert hasattr(L.Context, "set_locate_pairings")


def test_null_shape_and_offset_errors_need_no_device():
    import rust_kzg_bn254_amd as k
    L = k._lib
    lib = L.load()
    g1s, g2s = eip197_pairs()
    p1, p2 = L.ptr(g1s), L.ptr(g2s)
    ok, gt, bad = (C.c_uint8 * 4)(7, 7, 7, 7), (C.c_uint64 * (48 * 4))(), C.c_uint64(99)
    off = lambda *v: (C.c_uint64 * len(v))(*v)                       # noqa: E731
    fake = C.c_void_p(1)                     # every row below is decided before the context is touched: this one is never dereferenced
    for call, out in ((lib.kzg_pairings_product_verify_batch, ok), (lib.kzg_pairings_product_gt_batch, gt)):
        assert call(None, p1, p2, off(0, 2), 1, out, C.byref(bad)) == L.ERR_INVALID_ARG
        assert call(fake, p1, p2, None, 1, out, C.byref(bad)) == L.ERR_INVALID_ARG
        assert call(fake, p1, p2, off(0, 2), 1, None, C.byref(bad)) == L.ERR_INVALID_ARG
        assert call(fake, None, p2, off(0, 2), 1, out, None) == L.ERR_INVALID_ARG
        assert call(fake, p1, None, off(0, 2), 1, out, None) == L.ERR_INVALID_ARG
        assert call(fake, p1, p2, off(1, 2), 1, out, None) == L.ERR_INVALID_ARG            # does not start at 0
        assert call(fake, p1, p2, off(0, 2, 1), 2, out, None) == L.ERR_INVALID_ARG         # decreases
        assert call(fake, p1, p2, off(0, 65), 1, out, None) == L.ERR_TOO_LARGE             # more than 64 pairs in one check
        assert call(fake, p1, p2, off(0), (1 << 20) + 1, out, None) == L.ERR_TOO_LARGE     # (the count is judged before the offsets are read)
    assert bytes(ok) == b"\x07" * 4 and bad.value == 99 and not any(gt)
    assert lib.kzg_ctx_set_locate_pairings(None, 0) == L.ERR_INVALID_ARG
    # the host GT entry: nulls, and the EIP-197 product is one -- (R mod p, 0, .., 0) in Montgomery words
    one = (C.c_uint64 * 48)()
    assert lib.kzg_pairings_product_gt(p1, p2, 2, None) == L.ERR_INVALID_ARG and lib.kzg_pairings_product_gt(None, p2, 2, one) == L.ERR_INVALID_ARG
    gtv = k.verifier.pairings_product_gt(g1s, g2s)
    want = np.zeros((12, 4), np.uint64)
    want[0] = pyref.fq_to_mont(1)
    assert np.array_equal(gtv, want) and k.verifier.pairings_product_verify(g1s, g2s) is True
    assert np.array_equal(k.verifier.pairings_product_gt(g1s[:0], g2s[:0]), want)          # the empty product
    other = k.verifier.pairings_product_gt(g1s[:1], g2s[:1])
    assert not np.array_equal(other, want) and other.any()
    off1 = g1s.copy(); off1[0, 0] ^= np.uint64(1)
    off2 = g2s.copy(); off2[1, 3] ^= np.uint64(1)
    for a, b in ((off1, g2s), (g1s, off2), (off1, off2)):
        try:
            k.verifier.pairings_product_gt(a, b)
        except k.errors.NotOnCurveError as e:
            assert ("G1" in str(e)) == (a is off1)                    # the G1 error wins
        else:
            raise AssertionError("a point off its curve passed")
