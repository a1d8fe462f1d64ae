"""CPU-only checks of blob headers in their serialized form (`kzg_header_items_encode_be`, the host-compilable half of
`kzg_verify_length_proof_batch_bytes`):

* tests/hostcheck/headerbytescheck.cpp, a stand-alone program with its own main: csrc/header_item_stream.h (the block producer a lane of
  k_header_item_digests runs) compiled by g++ with every lazy-reduction bound an abort, all six blocks and the digest of each header
  against the item message of csrc/host_fiat_shamir.h, and the G2 encoder of csrc/host_header_bytes.h against the host decoder; built
  once plainly and once with AddressSanitizer and UBSan and run directly (nothing is loaded into Python under a sanitizer);
* `kzg_header_items_encode_be` through the library, byte for byte against tests/g2_compress_ref.py and `helpers.compress_g1_be`, with
  the identity, a coordinate not below p and the NULL-pair rules;
* the declarations of the four new entries against the library's exports and the ctypes prototypes;
* the argument errors of the device entries that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import g2_compress_ref
import pyref
from pyref import P, R_

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")
ENTRIES = ("kzg_header_items_encode_be", "kzg_header_items_decode_be", "kzg_verify_length_proof_batch_bytes", "kzg_verify_length_proof_batch_locate_bytes")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    return k


@pytest.mark.parametrize("flags", [["-O1"], SAN], ids=["plain", "sanitized"])
def test_item_stream_and_encoder_as_a_host_program(tmp_path, flags):
    exe = str(tmp_path / "headerbytescheck")
    subprocess.check_call(["g++", "-std=c++17", "-DKZG_BOUND_CHECK", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", *flags,
                           "-I" + CSRC, os.path.join(HERE, "hostcheck", "headerbytescheck.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    m = re.fullmatch(r"headerbytescheck ok (\d+) (\d+)", r.stdout.strip())
    assert r.returncode == 0 and m, (r.stdout[-500:], r.stderr[-3000:])
    # random headers, the eight negated ones, four identity patterns, the generator; coordinates with a zero top byte occurred
    assert int(m.group(1)) >= 40 + 8 + 4 + 1 and int(m.group(2)) >= 3


def test_host_headers_include_no_hip():
    for name in ("header_item_stream.h", "host_header_bytes.h"):
        src = open(os.path.join(CSRC, name)).read()
        includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
        assert includes and not any("hip" in inc or "engine" in inc for inc in includes), (name, includes)
    stream = open(os.path.join(CSRC, "header_item_stream.h")).read()
    fns = re.findall(r"^(\w[\w ]*?)\s+(header_item_\w+)\(", stream, re.M)
    assert len(fns) == 3 and all(ret.startswith("KZG_HD") for ret, _ in fns), fns


def some_headers(k, count):
    """wire points (c, c2, pi2) of `count` headers; any subgroup points do for the encoder"""
    c = np.stack([pyref.point_to_wire(pyref.ec_mul(3 * i + 2, (1, 2))) for i in range(count)])
    c2 = np.stack([k.helpers.g2_mul_generator(pyref.fr_to_mont((7 * i + 1) % R_)) for i in range(count)])
    pi2 = np.stack([k.helpers.g2_mul_generator(pyref.fr_to_mont(pow(5, i + 1, R_))) for i in range(count)])
    return c, c2, pi2


def test_encoder_against_the_python_compression_byte_for_byte(k):
    c, c2, pi2 = some_headers(k, 12)
    neg = g2_compress_ref.negate_wire(c2[:4])                       # the same x with the other y: both flags in one array
    c2 = np.concatenate([c2, neg])
    pi2 = np.concatenate([pi2, g2_compress_ref.negate_wire(pi2[:4])])
    c = np.concatenate([c, np.stack([pyref.point_to_wire(pyref.ec_neg(pyref.point_from_wire(w))) for w in c[:4]])])
    cb, c2b, p2b = k.verifier.encode_header_items(c, c2, pi2)
    assert cb == k.helpers.compress_g1_be(c)
    assert c2b == g2_compress_ref.compress_wire(c2) and p2b == g2_compress_ref.compress_wire(pi2)
    assert {b >> 6 for b in c2b[::64]} == {2, 3}
    assert k.helpers.compress_g2_be(c2) == c2b
    # the generator is an element like any other (f = 1)
    gen = k.helpers.g2_mul_generator(pyref.fr_to_mont(1))
    assert k.helpers.compress_g2_be(gen) == g2_compress_ref.compress_wire(gen)


def test_encoder_identity_and_refusals(k):
    L = k._lib
    lib = k.load()
    c, c2, pi2 = some_headers(k, 3)
    c[1] = 0; c2[1] = 0; pi2[2] = 0
    cb, c2b, p2b = k.verifier.encode_header_items(c, c2, pi2)
    assert cb[32:64] == b"\x40" + bytes(31)
    assert c2b[64:128] == b"\x40" + bytes(63) and p2b[128:192] == b"\x40" + bytes(63)
    assert c2b[:64] == g2_compress_ref.compress_wire(c2[0]) and p2b[:64] == g2_compress_ref.compress_wire(pi2[0])
    # a coordinate not below p, in each array and each G2 coordinate
    p_words = np.array([(P >> (64 * j)) & (2 ** 64 - 1) for j in range(4)], np.uint64)
    G = k.errors.GenericError
    for q in range(4):
        bad = c2.copy()
        bad[0, 4 * q:4 * q + 4] = p_words
        with pytest.raises(G, match="not below the modulus"):
            k.verifier.encode_header_items(c, bad, pi2)
        with pytest.raises(G, match="not below the modulus"):
            k.verifier.encode_header_items(None, None, bad)
    badc = c.copy()
    badc[0, 4:8] = p_words
    with pytest.raises(G, match="not below the modulus"):
        k.verifier.encode_header_items(badc, c2, pi2)
    # pairs may be NULL together; half a pair, or nothing at all with count > 0, is refused
    assert k.verifier.encode_header_items(c, None, None) == (cb, None, None)
    assert k.verifier.encode_header_items(None, c2, None) == (None, c2b, None)
    assert k.verifier.encode_header_items(None, None, pi2) == (None, None, p2b)
    assert k.verifier.encode_header_items(None, None, None) == (None, None, None)
    o32, o64 = np.zeros(96, np.uint8), np.zeros(192, np.uint8)
    u8 = lambda a: a.ctypes.data_as(L.u8p)                                      # noqa: E731
    P_ = L.ptr
    assert lib.kzg_header_items_encode_be(P_(c), P_(c2), P_(pi2), 3, u8(o32), u8(o64), None) == L.ERR_INVALID_ARG
    assert lib.kzg_header_items_encode_be(None, P_(c2), P_(pi2), 3, u8(o32), u8(o64), u8(o64)) == L.ERR_INVALID_ARG
    assert lib.kzg_header_items_encode_be(P_(c), None, None, 3, None, None, None) == L.ERR_INVALID_ARG
    assert lib.kzg_header_items_encode_be(None, None, None, 3, None, None, None) == L.ERR_INVALID_ARG
    assert lib.kzg_header_items_encode_be(None, None, None, 0, None, None, None) == L.OK
    assert lib.kzg_header_items_encode_be(P_(c), None, None, 2 ** 20 + 1, u8(o32), None, None) == L.ERR_TOO_LARGE
    with pytest.raises(k.errors.InvalidInputLength):
        k.verifier.encode_header_items(c, c2[:2], pi2)


def test_header_prototypes_and_exports_agree_on_the_new_entries(k):
    hdr = open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read()
    lib = C.CDLL(k._lib.LIB_PATH)
    L = k._lib
    params = {}
    for name in ENTRIES:
        decl = re.search(r"\bint32_t %s\s*\(([^;]*)\);" % name, hdr)
        assert decl, name
        assert name in L.PROTOTYPES and hasattr(lib, name), name
        params[name] = [re.sub(r"/\*.*?\*/", "", p).split()[-1].lstrip("*") for p in decl.group(1).split(",")]
        assert len(params[name]) == len(L.PROTOTYPES[name][1]), name
    batch = L.PROTOTYPES["kzg_verify_length_proof_batch"][1]
    locate = L.PROTOTYPES["kzg_verify_length_proof_batch_locate"][1]
    i32p, u64ptr = C.POINTER(L.i32), C.POINTER(C.c_uint64)
    as_bytes = lambda args: [args[0]] + [L.u8p] * 3 + list(args[4:])            # noqa: E731
    # the decoded entries with the three point arrays as bytes, out_weights_mont behind out_ok, bad_array at the end
    assert L.PROTOTYPES["kzg_verify_length_proof_batch_bytes"] == (L.i32, as_bytes(batch[:11]) + [L.u64p, u64ptr, i32p])
    assert L.PROTOTYPES["kzg_verify_length_proof_batch_locate_bytes"] == (L.i32, as_bytes(locate) + [i32p])
    head = ["ctx", "commitments_be", "length_commitments_be", "length_proofs_be", "claimed_lens", "count", "shift_lens", "g1_tau_shifts_xy", "n_shifts", "weights_mont"]
    assert params["kzg_verify_length_proof_batch_bytes"] == head + ["out_ok", "out_weights_mont", "bad_index", "bad_array"]
    assert params["kzg_verify_length_proof_batch_locate_bytes"] == head + ["group_indices", "n_groups", "out_group_ok", "out_bad_groups", "out_pairing_checks",
                                                                            "bad_index", "bad_array"]
    assert params["kzg_header_items_decode_be"] == ["ctx"] + head[1:4] + ["count", "out_commitments_xy", "out_length_commitments", "out_length_proofs", "bad_index",
                                                                          "bad_array"]
    assert params["kzg_header_items_encode_be"] == ["commitments_xy", "length_commitments", "length_proofs", "count", "out_commitments_be",
                                                    "out_length_commitments_be", "out_length_proofs_be"]
    # the decoder of SRS files keeps its own flag rule: no identity bit was added to it
    assert "KZG_G2_ACCEPT_IDENTITY" not in hdr and re.search(r"#define KZG_G2_REJECT_GENERATOR 2u", hdr)


def test_python_surface_names_the_new_entries(k):
    for fn, entry in ((k.verifier.encode_header_items, "kzg_header_items_encode_be"), (k.verifier.decode_header_items, "kzg_header_items_decode_be"),
                      (k.verifier.verify_length_proof_batch_bytes, "kzg_verify_length_proof_batch_bytes"),
                      (k.verifier.locate_bad_headers_bytes, "kzg_verify_length_proof_batch_locate_bytes"), (k.helpers.compress_g2_be, "kzg_header_items_encode_be"),
                      (k.KZG.commit_with_length_proof_batch_be, "encode_header_items")):
        assert entry in fn.__doc__, fn.__name__


def test_argument_errors_that_need_no_device(k):
    """The null context is the first check of the three device entries: every call below returns before it needs a device and writes no
    output.  The Python surface refuses its own argument errors without creating a context."""
    lib = k.load()
    L = k._lib
    b32, b64 = np.zeros(32, np.uint8), np.zeros(64, np.uint8)
    b32[0] = b64[0] = 0x40
    g1 = np.zeros((1, 8), np.uint64)
    lens = np.array([4], np.uint64)
    idx = np.zeros(1, np.uint64)
    o8, o16 = np.full((1, 8), 7, np.uint64), np.full((1, 16), 7, np.uint64)
    flag = np.full(1, 7, np.uint8)
    ok, arr, n_bad, checks, bad = L.i32(7), L.i32(7), L.sz(7), L.sz(7), C.c_uint64(7)
    u8 = lambda a: a.ctypes.data_as(L.u8p)                                      # noqa: E731
    P_ = L.ptr
    assert lib.kzg_header_items_decode_be(None, u8(b32), u8(b64), u8(b64), 1, P_(o8), P_(o16), P_(o16), C.byref(bad), C.byref(arr)) == L.ERR_INVALID_ARG
    assert lib.kzg_verify_length_proof_batch_bytes(None, u8(b32), u8(b64), u8(b64), P_(lens), 1, P_(lens), P_(g1), 1, None, C.byref(ok), None, C.byref(bad),
                                                   C.byref(arr)) == L.ERR_INVALID_ARG
    assert lib.kzg_verify_length_proof_batch_bytes(None, None, None, None, None, 0, None, None, 0, None, None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.kzg_verify_length_proof_batch_locate_bytes(None, u8(b32), u8(b64), u8(b64), P_(lens), 1, P_(lens), P_(g1), 1, None, P_(idx), 1, u8(flag),
                                                          C.byref(n_bad), C.byref(checks), C.byref(bad), C.byref(arr)) == L.ERR_INVALID_ARG
    assert (o8 == 7).all() and (o16 == 7).all() and flag[0] == 7 and (ok.value, arr.value, n_bad.value, checks.value, bad.value) == (7, 7, 7, 7, 7)
    before = dict(L._default_ctx)                                               # device id -> Context: must not grow
    shifts = {4: g1[0]}
    V = k.verifier
    with pytest.raises(k.errors.InvalidInputLength):
        V.verify_length_proof_batch_bytes(bytes(b32), bytes(b64) * 2, bytes(b64), [4], shifts)
    with pytest.raises(k.errors.InvalidInputLength):
        V.verify_length_proof_batch_bytes(bytes(b32)[:31], bytes(b64), bytes(b64), [4], shifts)
    with pytest.raises(k.errors.InvalidInputLength):
        V.verify_length_proof_batch_bytes(bytes(b32), bytes(b64), bytes(b64), [4], shifts, weights=pyref.frs_to_mont([1]))
    with pytest.raises(k.errors.InvalidInputLength):
        V.decode_header_items(bytes(b32), bytes(b64), bytes(b64) * 2)
    with pytest.raises(k.errors.GenericError, match="not the same"):
        V.locate_bad_headers_bytes(bytes(b32), bytes(b64), bytes(b64), [4], shifts, groups=[0, 0], n_groups=1)
    with pytest.raises(k.errors.GenericError, match="item"):
        V.locate_bad_headers_bytes(bytes(b32), bytes(b64), bytes(b64), [4], shifts, groups="commitment")
    assert V.decode_header_items(b"", b"", b"")[1].shape == (0, 16)
    assert L._default_ctx == before
