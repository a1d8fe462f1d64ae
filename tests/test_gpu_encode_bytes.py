"""-m gpu: the disperser's half on bytes -- `kzg_encode_cosets_batch_bytes` (blobs decoded where the group's first kernel loads them, values
encoded where the gather kernel stores them, proofs compressed by the affine conversion behind FK20) and `kzg_disperse_blobs_bytes` (the
same plus the blob headers from the same resident coefficients).

The reference everywhere is the composition a caller had before: host decode of the blob, `kzg_encode_cosets_batch`,
`kzg_commit_coeff_form_batch`, `kzg_commit_with_length_proof_batch`, then the host encoders, compared byte for byte.  Behind it one fixed
input is pinned by big integers alone (values by evaluation, proofs by the closed form [(f(tau) - I_k(tau)) / (tau^l - w^(k l))] G with
the known tau) and by a SHA-256 digest of that reference's bytes (PIN).  Shapes (d, n, l): (16, 32, 1), (16, 64, 8), (2048, 4096, 16) --
the last crosses 2^10, where the transforms' workspace changes; both forms; B in {1, 3}; B = 5 in three groups and in groups of one."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import coset_ref
import pyref
import recover_ref
from coset_bytes_ref import compress_be
from pyref import R_

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
u8p = C.POINTER(C.c_uint8)
TAU = int.from_bytes(hashlib.sha256(b"kzg-bn254-mi355x/encode-bytes/v1").digest(), "big") % R_
SRS_ORDER = 1 << 16
TRAIL = 4096
SHAPES = [(16, 32, 1), (16, 64, 8), (2048, 4096, 16)]
SENTINEL = 0xA5
ID32 = b"\x40" + bytes(31)
# sha256 over commitments || values || proofs (the entry's three outputs, in that order) that pin_reference() gives for pin_inputs():
# computed once from the big-integer reference alone
PIN = "97c44e4d71608ec49811764cca95a10665f46e21512551b797ff78b5cce877fc"


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


class World:
    pass


@pytest.fixture(scope="module")
def world(k):
    w = World()
    w.srs = k.SRS.generate(TAU, 2048)
    w.kz = k.KZG.new()
    w.g2 = k.G2SRS.generate(TAU, 2048)
    w.trailing = k.G2SRS.generate(TAU, TRAIL, first_power=SRS_ORDER - TRAIL)
    w.cache = {}
    yield w
    for h in (w.srs, w.g2, w.trailing):
        h.close()


def be(ints):
    return b"".join(int(v).to_bytes(32, "big") for v in ints)


def coeff_rows(B, d, seed):
    """B x d coefficients; blob 0 starts with 0, 1, r - 1"""
    rnd = random.Random("encode-bytes/%s" % (seed,))
    rows = [[rnd.randrange(R_) for _ in range(d)] for _ in range(B)]
    rows[0][:3] = [0, 1, R_ - 1]
    return rows


def blobs_of(rows, ef):
    """the blobs' bytes in the form the call takes: coefficients, or evaluations on the d-point domain"""
    return b"".join(be(recover_ref.fft(r) if ef else r) for r in rows)


def composition(k, w, rows, n, l, ef, key=None):
    """(commitments_be, ys_be, proofs_be) by the route a caller had: words up, words down, host encoders"""
    if key is not None and key in w.cache:
        return w.cache[key]
    B, d = len(rows), len(rows[0])
    coeffs = [k.PolynomialCoeffForm(pyref.frs_to_mont(r)) for r in rows]
    if ef:
        data = np.ascontiguousarray(np.stack([pyref.frs_to_mont(recover_ref.fft(r)) for r in rows]))
    else:
        data = np.ascontiguousarray(np.stack([p.coeffs() for p in coeffs]))
    ys, proofs = w.kz.encode_cosets_batch(data.reshape(B, d, 4), w.srs, n, l, eval_form=bool(ef))
    ys_be, pf_be = k.verifier.encode_coset_items(ys.reshape(-1, l, 4), proofs.reshape(-1, 8))
    cm_be = k.helpers.compress_g1_be(w.kz.commit_coeff_form_batch(coeffs, w.srs))
    out = (cm_be, ys_be, pf_be)
    if key is not None:
        w.cache[key] = out
    return out


def fused(k, ctx, srs, blobs_be, B, d, n, l, ef, want=(True, True, True)):
    """The C-ABI entry: (status, commitments, values, proofs, bad index); outputs start from a sentinel, an output not asked for is None."""
    L = k._lib
    buf = np.frombuffer(blobs_be, np.uint8)
    m = n // l
    outs = [np.full(size, SENTINEL, dtype=np.uint8) if on else None for on, size in zip(want, (B * 32, B * n * 32, B * m * 32))]
    p8 = lambda a: None if a is None else a.ctypes.data_as(u8p)
    bad = C.c_uint64(1 << 40)
    rc = L.load().kzg_encode_cosets_batch_bytes(ctx.handle, srs.handle, buf.ctypes.data_as(u8p), B, d, ef, n, l, p8(outs[0]), p8(outs[1]), p8(outs[2]), C.byref(bad))
    return (rc,) + tuple(None if a is None else a.tobytes() for a in outs) + (bad.value,)


# ---- 1. byte identity with the composition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("ef", [0, 1])
@pytest.mark.parametrize("d,n,l", SHAPES)
def test_byte_identity_with_the_composition(k, world, d, n, l, ef, B):
    ctx = k.default_context()
    rows = coeff_rows(B, d, (d, n, l, B))
    want = composition(k, world, rows, n, l, ef)
    blobs = blobs_of(rows, ef)
    rc, cm, ys, pf, _ = fused(k, ctx, world.srs, blobs, B, d, n, l, ef)
    assert rc == 0 and (cm, ys, pf) == want
    for i in range(3):                                                                  # each output alone
        only = tuple(j == i for j in range(3))
        got = fused(k, ctx, world.srs, blobs, B, d, n, l, ef, only)
        assert got[0] == 0 and got[1 + i] == want[i] and all(got[1 + j] is None for j in range(3) if j != i), (i,)
    # the Python surface, from bytes, from Blob objects and from an array
    kz = world.kz
    if B == 1:
        assert kz.encode_cosets_batch_bytes(blobs, world.srs, n, l, eval_form=bool(ef)) == want
    per = d * 32
    as_list = [blobs[b * per:(b + 1) * per] for b in range(B)]
    assert kz.encode_cosets_batch_bytes(as_list, world.srs, n, l, eval_form=bool(ef)) == want
    arr = np.frombuffer(blobs, np.uint8).reshape(B, per)
    assert kz.encode_cosets_batch_bytes(arr, world.srs, n, l, eval_form=bool(ef), commitments=False) == (None,) + want[1:]
    if d == 16 and B == 3:
        assert kz.encode_cosets_batch_bytes([k.Blob.from_padded_unchecked(b) for b in as_list], world.srs, n, l, eval_form=bool(ef), values=False,
                                            proofs=False) == (want[0], None, None)


@pytest.mark.parametrize("ef", [0, 1])
def test_groups_give_the_same_bytes(k, world, ef):
    L = k._lib
    ctx = L.Context(0)
    d, n, l, B = 2048, 4096, 16, 5
    srs = k.SRS.generate(TAU, d, ctx=ctx)                                               # (the group budget is the context's)
    info = k.helpers.encode_batch_info
    two = info(d, n, l, 2)["group_bytes"]
    assert info(d, n, l, B)["groups"] == 1
    assert (info(d, n, l, B, group_bytes=two)["groups"], info(d, n, l, B, group_bytes=two)["blobs_per_group"]) == (3, 2)
    assert (info(d, n, l, B, group_bytes=1)["groups"], info(d, n, l, B, group_bytes=1)["blobs_per_group"]) == (B, 1)
    rows = coeff_rows(B, d, "groups")
    blobs = blobs_of(rows, ef)
    ctx.set_encode_group_bytes(0)
    rc, *one_group, _ = fused(k, ctx, srs, blobs, B, d, n, l, ef)
    assert rc == 0 and tuple(one_group) == composition(k, world, rows, n, l, ef, key=("groups", ef))
    for budget in (two, 1):                                                             # three groups; groups of one (multiproof_encode's launches)
        ctx.set_encode_group_bytes(budget)
        rc, *got, _ = fused(k, ctx, srs, blobs, B, d, n, l, ef)
        assert rc == 0 and got == one_group, budget
    srs.close()
    ctx.close()


def test_edge_rows_inside_a_batch(k, world):
    ctx = k.default_context()
    d, n, l, B = 16, 64, 8, 4
    m = n // l
    rows = coeff_rows(B, d, "edges/1")          # (at d = 2 l every coset of a blob has the same quotient: two distinct proofs here, and this seed gives both signs)
    rows = [[0] * d, [12345] + [0] * (d - 1), rows[0], rows[1]]                         # zero, constant, (0, 1, r - 1, ..), random
    want = composition(k, world, rows, n, l, 0)
    rc, cm, ys, pf, _ = fused(k, ctx, world.srs, blobs_of(rows, 0), B, d, n, l, 0)
    assert rc == 0 and (cm, ys, pf) == want
    assert cm[:32] == ID32 and pf[:m * 32] == ID32 * m and ys[:n * 32] == bytes(n * 32)   # the zero blob
    assert pf[m * 32:2 * m * 32] == ID32 * m and cm[32] >> 6 in (2, 3)                  # a constant: no quotient, a finite commitment
    assert ys[n * 32:2 * n * 32] == be([12345]) * n
    flags = {pf[32 * i] >> 6 for i in range(2 * m, 4 * m)}
    assert flags == {2, 3}                                                              # both signs occur among the proofs (the seed is chosen so)


# ---- 2. one input pinned by big integers alone ----------------------------------------------------------------------------------------------
def pin_inputs():
    d, n, l, B = 16, 32, 1, 2
    rnd = random.Random("encode-bytes/pin/v1")
    return d, n, l, B, [[rnd.randrange(R_) for _ in range(d)] for _ in range(B)]


def reference_bytes(rows, n, l):
    """(commitments_be, ys_be, proofs_be) from big integers: values by evaluation, proofs by the closed form at the known tau"""
    m = n // l
    w = pyref.root_of_unity(n.bit_length() - 1)
    g1 = lambda s: compress_be(pyref.ec_mul(s % R_, pyref.G1) if s % R_ else None)
    cm, ys_be, pf = [], [], []
    for f in rows:
        f_tau = pyref.poly_eval(f, TAU)
        cm.append(g1(f_tau))
        for k_ in range(m):
            ys = [pyref.poly_eval(f, pow(w, k_ + j * m, R_)) for j in range(l)]
            ys_be.append(be(ys))
            i_tau = pyref.poly_eval(coset_ref.interpolation_coeffs(ys, k_, n), TAU)
            q_tau = (f_tau - i_tau) * pow((pow(TAU, l, R_) - pow(w, k_ * l, R_)) % R_, -1, R_)
            pf.append(g1(q_tau))
    return b"".join(cm), b"".join(ys_be), b"".join(pf)


def pin_reference_digest():
    d, n, l, B, rows = pin_inputs()
    return hashlib.sha256(b"".join(reference_bytes(rows, n, l))).hexdigest()


def test_the_reference_digest_is_reproduced(k, world):
    d, n, l, B, rows = pin_inputs()
    ref = reference_bytes(rows, n, l)
    assert hashlib.sha256(b"".join(ref)).hexdigest() == PIN                             # the pin is the reference's, whatever the library does
    assert composition(k, world, rows, n, l, 0) == ref                                  # the route a caller had
    rc, *got, _ = fused(k, k.default_context(), world.srs, blobs_of(rows, 0), B, d, n, l, 0)
    assert rc == 0 and tuple(got) == ref                                                # the new entry
    rc, *got, _ = fused(k, k.default_context(), world.srs, blobs_of(rows, 1), B, d, n, l, 1)
    assert rc == 0 and tuple(got) == ref                                                # ... and from the evaluations of the same polynomials


# ---- 3. round trip through the other legs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,l", [(16, 64, 8), (2048, 4096, 16)])
def test_the_bytes_verify_and_half_of_them_give_the_blobs_back(k, world, d, n, l):
    B, m = 3, n // l
    rows = coeff_rows(B, d, ("round trip", d))
    blobs = blobs_of(rows, 0)
    cm, ys, pf = world.kz.encode_cosets_batch_bytes([blobs[b * d * 32:(b + 1) * d * 32] for b in range(B)], world.srs, n, l)
    g2 = k.helpers.g2_mul_generator(k.fr.fr_from_int(pow(TAU, l, R_)))
    ci = [b for b in range(B) for _ in range(m)]
    ki = [c for _ in range(B) for c in range(m)]
    assert k.verifier.verify_multiproof_batch_bytes(cm, ci, ki, ys, pf, n, l, world.srs, g2) is True
    flipped = bytearray(ys); flipped[-1] ^= 1
    assert k.verifier.verify_multiproof_batch_bytes(cm, ci, ki, bytes(flipped), pf, n, l, world.srs, g2) is False
    rnd = random.Random(d)
    pick = np.array([sorted(rnd.sample(range(m), m // 2)) for _ in range(B)], dtype=np.uint64)
    half_y = b"".join(ys[(b * m + int(c)) * l * 32:(b * m + int(c) + 1) * l * 32] for b in range(B) for c in pick[b])
    half_p = b"".join(pf[(b * m + int(c)) * 32:(b * m + int(c) + 1) * 32] for b in range(B) for c in pick[b])
    ok, polys, consistent = k.verifier.retrieve_blobs_bytes(cm, pick, half_y, half_p, n, l, world.srs, g2, degree_bound=d, eval_form=False, out_len=d)
    assert ok is True and polys == blobs and consistent.all()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def with_value(blobs_be, at, v):
    b = bytearray(blobs_be)
    b[32 * at:32 * at + 32] = int(v).to_bytes(32, "big")
    return bytes(b)


@pytest.mark.parametrize("ef", [0, 1])
def test_a_value_not_below_r_is_refused_with_its_place(k, world, ef):
    L = k._lib
    ctx = L.Context(0)
    d, n, l, B = 16, 64, 8, 5
    m = n // l
    srs = k.SRS.generate(TAU, d, ctx=ctx)
    two = k.helpers.encode_batch_info(d, n, l, 2)["group_bytes"]
    assert k.helpers.encode_batch_info(d, n, l, B, group_bytes=two)["blobs_per_group"] == 2
    ctx.set_encode_group_bytes(two)                                                     # groups {0, 1}, {2, 3}, {4}
    rows = coeff_rows(B, d, "refusals")
    good = blobs_of(rows, ef)
    rc, *want, _ = fused(k, ctx, srs, good, B, d, n, l, ef)
    assert rc == 0 and tuple(want) == composition(k, world, rows, n, l, ef)
    sentinel = bytes([SENTINEL])
    # blob 0: nothing leaves
    rc, cm, ys, pf, bad = fused(k, ctx, srs, with_value(good, 5, R_), B, d, n, l, ef)
    assert (rc, bad) == (L.ERR_DESERIALIZE, 5) and set(cm + ys + pf) == {SENTINEL}
    assert "value 5" in ctx.last_error()
    # the last blob of the second group, and one behind it in the third: the first group's outputs are written, the later groups' are not
    at = 3 * d + d - 1
    both = with_value(with_value(good, at, 2 ** 256 - 1), 4 * d + 1, R_)
    rc, cm, ys, pf, bad = fused(k, ctx, srs, both, B, d, n, l, ef)
    assert (rc, bad) == (L.ERR_DESERIALIZE, at)
    for got, exp, per in ((cm, want[0], 32), (ys, want[1], n * 32), (pf, want[2], m * 32)):
        assert got[:2 * per] == exp[:2 * per] and got[2 * per:] == sentinel * (3 * per)
    # two bad values in one group: the smaller place
    two_bad = with_value(with_value(good, 2 * d + 9, R_ + 5), 2 * d + 3, R_)
    assert fused(k, ctx, srs, two_bad, B, d, n, l, ef)[0::4] == (L.ERR_DESERIALIZE, 2 * d + 3)
    # r + 1 with the top bits set is refused, not reduced; r - 1 decodes; groups of one report the same place
    assert fused(k, ctx, srs, with_value(good, at, (R_ + 1) | (3 << 254)), B, d, n, l, ef)[0::4] == (L.ERR_DESERIALIZE, at)
    ctx.set_encode_group_bytes(1)
    assert fused(k, ctx, srs, with_value(good, at, R_ + 1), B, d, n, l, ef)[0::4] == (L.ERR_DESERIALIZE, at)
    rc, *got, _ = fused(k, ctx, srs, good, B, d, n, l, ef)                              # the same call works afterwards
    assert rc == 0 and got == want
    kz = k.KZG.new(ctx)
    with pytest.raises(k.errors.SerializationError, match=r"blob 3, element %d\b" % (d - 1)):
        kz.encode_cosets_batch_bytes(np.frombuffer(with_value(good, at, R_), np.uint8).reshape(B, d * 32), srs, n, l, eval_form=bool(ef))
    srs.close()
    ctx.close()


def test_the_table_of_the_words_entry_then_the_cap(k, world):
    L = k._lib
    ctx = k.default_context()
    blobs = bytes(3 * 16 * 32)
    f = lambda *a, **kw: fused(k, ctx, world.srs, blobs, *a, **kw)[0]
    assert f(3, 16, 48, 1, 0) == L.ERR_NOT_POWER_OF_TWO
    assert f(3, 16, 32, 16, 0) == L.ERR_INVALID_ARG and f(3, 16, 8, 1, 0) == L.ERR_INVALID_ARG
    assert f(1, 4096, 8192, 1, 0) == L.ERR_SRS_CAPACITY_EXCEEDED
    assert f(3, 16, 32, 1, 0, want=(False, False, False)) == L.ERR_INVALID_ARG
    z = (C.c_uint8 * 64)()                                                              # count x poly_len > 2^28: before anything is read or written
    assert L.load().kzg_encode_cosets_batch_bytes(ctx.handle, world.srs.handle, z, (1 << 28) // 16 + 1, 16, 0, 32, 1, z, z, z, None) == L.ERR_TOO_LARGE
    assert L.load().kzg_encode_cosets_batch_bytes(ctx.handle, world.srs.handle, z, 3, 16, 0, 1 << 25, 1, z, z, z, None) == L.ERR_DOMAIN
    rc, cm, ys, pf, _ = fused(k, ctx, world.srs, blobs, 3, 16, 32, 3, 0)
    assert rc == L.ERR_INVALID_ARG and set(cm + ys + pf) == {SENTINEL}


# ---- 5. kzg_disperse_blobs_bytes ------------------------------------------------------------------------------------------------------------
def header_composition(k, w, rows, claimed):
    polys = [k.PolynomialCoeffForm(pyref.frs_to_mont(r)) for r in rows]
    return w.kz.commit_with_length_proof_batch_be(polys, w.srs, w.g2, w.trailing, SRS_ORDER, claimed)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("d,n,l", [(16, 64, 8), (2048, 4096, 16)])
def test_disperse_gives_the_headers_and_the_chunks_of_the_composition(k, world, d, n, l, B):
    w = world
    rows = coeff_rows(B, d, ("disperse", d, B))
    blobs = blobs_of(rows, 0)
    chunks = composition(k, w, rows, n, l, 0)
    for claimed in (d, 2 * d):
        hdr = header_composition(k, w, rows, claimed)
        assert hdr[0] == chunks[0]
        # with the values the coefficient rows are n apart (f_stride > d); proofs alone leave them compact (f_stride = d)
        got = w.kz.disperse_blobs_bytes(np.frombuffer(blobs, np.uint8).reshape(B, d * 32), w.srs, w.g2, w.trailing, SRS_ORDER, claimed, n, l)
        assert got == hdr + chunks[1:], claimed
        got = w.kz.disperse_blobs_bytes(np.frombuffer(blobs, np.uint8).reshape(B, d * 32), w.srs, w.g2, w.trailing, SRS_ORDER, claimed, n, l, values=False)
        assert got == hdr + (None, chunks[2])
        shift = k.SRS.generate(TAU, 1, first_power=SRS_ORDER - claimed)
        assert k.verifier.verify_length_proof_batch_bytes(*hdr, [claimed] * B, {claimed: shift.g1[0].copy()}) is True
        shift.close()
    # the header alone, from a domain of the polynomial's own length (n = d: nothing to place)
    got = w.kz.disperse_blobs_bytes([blobs[b * d * 32:(b + 1) * d * 32] for b in range(B)], w.srs, w.g2, w.trailing, SRS_ORDER, d, d, l, values=False, proofs=False)
    assert got == header_composition(k, w, rows, d) + (None, None)


def test_disperse_refusals(k, world):
    w = world
    d, n, l, B = 16, 64, 8, 3
    rows = coeff_rows(B, d, "disperse refusals")
    blobs = blobs_of(rows, 0)
    arr = lambda b: np.frombuffer(b, np.uint8).reshape(B, d * 32)
    call = lambda b, claimed: w.kz.disperse_blobs_bytes(arr(b), w.srs, w.g2, w.trailing, SRS_ORDER, claimed, n, l)
    with pytest.raises(k.errors.FFTError):
        call(blobs, 24)                                                                 # claimed_len not a power of two
    with pytest.raises(k.errors.GenericError):
        call(blobs, 8)                                                                  # poly_len > claimed_len
    with pytest.raises(k.errors.SrsCapacityExceeded):
        call(blobs, 2 * TRAIL)                                                          # the trailing powers do not reach that far down
    with pytest.raises(k.errors.SerializationError, match=r"blob 2, element 7\b"):
        call(with_value(blobs, 2 * d + 7, R_), d)
    assert call(blobs, d) == header_composition(k, w, rows, d) + composition(k, w, rows, n, l, 0)[1:]


# ---- 6. the bound-checked build runs identity cases above with every site counter at 0 ----------------------------------------------------
VARIANT = os.path.join(ROOT, "rust-kzg-bn254_amd", "libkzg_bn254_mi355x_boundcheck.so")
CHILD = r'''
import ctypes as C, os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import torch  # noqa: F401  (load order: tests/conftest.py)
import rust_kzg_bn254_amd  # noqa: F401
L = [m for name, m in list(sys.modules.items()) if name.endswith("_lib") and hasattr(m, "LIB_PATH")][0]
assert L.LIB_PATH == os.environ["KZG_LIB_PATH"], L.LIB_PATH
h = L.load()
n = h.kzg_bc_sites()
assert h.kzg_bc_reset_all() == 0
import pytest
rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", "-x", "tests/test_gpu_encode_bytes.py", "-k",
                  "(byte_identity and 16-) or edge_rows or reference_digest"])
counts = (C.c_ulonglong * n)()
first = (C.c_int32 * (9 * n))()
assert h.kzg_bc_read_all(counts, first) == 0
print("PYTEST_RC", int(rc))
for s in range(n):
    print("SITE", s, counts[s])
'''


def test_bound_checked_build_keeps_every_precondition():
    assert os.path.exists(VARIANT), "make -C rust-kzg-bn254_amd/csrc boundcheck (__graft_entry__.build() does it)"
    env = dict(os.environ, KZG_LIB_PATH=VARIANT)
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0 and "PYTEST_RC 0" in out, (out[-3000:], res.stderr[-2000:])
    assert " passed" in out and "no tests ran" not in out, out[-1000:]
    sites = [ln.split() for ln in out.splitlines() if ln.startswith("SITE ")]
    assert sites
    fired = {int(s[1]): int(s[2]) for s in sites if int(s[2])}
    assert not fired, fired
