"""Mirror of the reference's `rust-kzg-bn254-verifier` crate (verifier/src/verify.rs, verifier/src/batch.rs).

The O(1) pairing check runs on the host inside the library (csrc/host_pairing.h); the data-parallel parts — barycentric
evaluation of every blob and the three n-point linear combinations of batch verification — run on the GPU through the
same C-ABI as the prover."""
import ctypes as C
import hashlib

import numpy as np

from . import _lib, helpers
from .consts import BYTES_PER_FIELD_ELEMENT, FR_MODULUS, RANDOM_CHALLENGE_KZG_BATCH_DOMAIN
from .errors import DeserializationError, GenericError, InvalidInputLength, NotOnCurveError
from .fr import fr_from_int, fr_to_int


def _raise_for(rc, ctx=None):
    if rc == _lib.OK:
        return
    if rc == _lib.ERR_G1_NOT_ON_CURVE:
        raise NotOnCurveError("G1 point not on curve")
    if rc == _lib.ERR_G2_TAU_NOT_ON_CURVE:
        raise NotOnCurveError("Invalid trusted setup: G2_TAU not on curve")
    if rc == _lib.ERR_TAU_EQUALS_Z:
        raise GenericError("Evaluation point equals trusted setup secret")
    if ctx is not None:
        ctx.check_device(rc)
    raise GenericError(_lib.status_message(rc))


def _g2_arg(g2_tau):
    return None if g2_tau is None else _lib.ptr(_lib.as_u64(g2_tau, 0).reshape(16))


def verify_proof(commitment, proof, value_fr, z_fr, g2_tau=None) -> bool:
    """verify.rs:10-72.  `g2_tau=None` uses consts::G2_TAU like the reference; tests with a generated SRS pass their own."""
    ok = _lib.i32(0)
    tau = None if g2_tau is None else _lib.as_u64(g2_tau, 0).reshape(16)
    rc = _lib.load().kzg_verify_proof(_lib.ptr(_lib.as_u64(commitment, 0).reshape(8)), _lib.ptr(_lib.as_u64(proof, 0).reshape(8)),
                                      _lib.ptr(_lib.as_u64(value_fr, 0).reshape(4)), _lib.ptr(_lib.as_u64(z_fr, 0).reshape(4)),
                                      None if tau is None else _lib.ptr(tau), C.byref(ok))
    _raise_for(rc)
    return bool(ok.value)


def verify_length_proof(commitment, length_commitment, length_proof, g1_tau_shift) -> bool:
    """The blob header's two pairing checks (`kzg_verify_length_proof`, host): e(C, G2) = e(G1, C2) and e([tau^(N-d)]_1, C2) = e(G1, pi2)
    with g1_tau_shift = [tau^(N-d)]_1 for the claimed length d over a setup of order N.  False = a check failed."""
    ok = _lib.i32(0)
    rc = _lib.load().kzg_verify_length_proof(_lib.ptr(_lib.as_u64(commitment, 0).reshape(8)), _lib.ptr(_lib.as_u64(length_commitment, 0).reshape(16)),
                                             _lib.ptr(_lib.as_u64(length_proof, 0).reshape(16)), _lib.ptr(_lib.as_u64(g1_tau_shift, 0).reshape(8)), C.byref(ok))
    if rc == _lib.ERR_G2_TAU_NOT_ON_CURVE:
        raise NotOnCurveError("G2 point not on curve")
    _raise_for(rc)
    return bool(ok.value)


def pairings_product_verify(g1s, g2s) -> bool:
    """prod_k e(g1s[k], g2s[k]) == 1 for any number of pairs (`kzg_pairings_product_verify`, host; EIP-197's predicate).  Pairs with an
    identity point contribute 1."""
    p1 = np.ascontiguousarray(_lib.as_u64(g1s, 8)).reshape(-1, 8)
    p2 = np.ascontiguousarray(_lib.as_u64(g2s, 16)).reshape(-1, 16)
    if len(p1) != len(p2):
        raise InvalidInputLength()
    ok = _lib.i32(0)
    rc = _lib.load().kzg_pairings_product_verify(_lib.ptr(p1) if len(p1) else None, _lib.ptr(p2) if len(p2) else None, len(p1), C.byref(ok))
    if rc == _lib.ERR_G2_TAU_NOT_ON_CURVE:
        raise NotOnCurveError("G2 point not on curve")
    _raise_for(rc)
    return bool(ok.value)


def _pairing_batch_args(g1s, g2s, offsets):
    p1 = np.ascontiguousarray(_lib.as_u64(g1s, 8)).reshape(-1, 8)
    p2 = np.ascontiguousarray(_lib.as_u64(g2s, 16)).reshape(-1, 16)
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64).reshape(-1))
    if len(p1) != len(p2) or len(off) == 0 or int(off[-1]) != len(p1):
        raise InvalidInputLength()
    return p1, p2, off


def _raise_for_pair(rc, bad, ctx):
    if rc == _lib.ERR_G1_NOT_ON_CURVE:
        raise NotOnCurveError("G1 point %d not on curve" % bad.value)
    if rc == _lib.ERR_G2_TAU_NOT_ON_CURVE:
        raise NotOnCurveError("G2 point %d not on curve" % bad.value)
    _raise_for(rc, ctx)


def pairings_product_verify_batch(g1s, g2s, offsets, ctx=None) -> np.ndarray:
    """`len(offsets) - 1` independent pairing-product checks in one launch on the device (`kzg_pairings_product_verify_batch`): check i
    covers the pairs offsets[i] .. offsets[i + 1] (offsets[0] = 0, never decreasing, offsets[-1] = the number of pairs) and entry i of the
    returned bool array is what `pairings_product_verify` returns for that slice.  An empty slice gives True."""
    p1, p2, off = _pairing_batch_args(g1s, g2s, offsets)
    ctx = ctx or _lib.default_context()
    n = len(off) - 1
    ok = np.zeros(max(n, 1), dtype=np.uint8)
    bad = C.c_uint64(0)
    rc = _lib.load().kzg_pairings_product_verify_batch(ctx.handle, _lib.ptr(p1) if len(p1) else None, _lib.ptr(p2) if len(p2) else None, _lib.ptr(off), n,
                                                       ok.ctypes.data_as(_lib.u8p), C.byref(bad))
    _raise_for_pair(rc, bad, ctx)
    return ok[:n].astype(bool)


def pairings_product_gt_batch(g1s, g2s, offsets, ctx=None) -> np.ndarray:
    """The value of every check of `pairings_product_verify_batch` (`kzg_pairings_product_gt_batch`): (n_checks, 12, 4) uint64, the
    final-exponentiated product as twelve Montgomery coefficients in the host's flat order; zeros where the Miller loop was degenerate."""
    p1, p2, off = _pairing_batch_args(g1s, g2s, offsets)
    ctx = ctx or _lib.default_context()
    n = len(off) - 1
    gt = np.zeros((max(n, 1), 12, 4), dtype=np.uint64)
    bad = C.c_uint64(0)
    rc = _lib.load().kzg_pairings_product_gt_batch(ctx.handle, _lib.ptr(p1) if len(p1) else None, _lib.ptr(p2) if len(p2) else None, _lib.ptr(off), n, _lib.ptr(gt),
                                                   C.byref(bad))
    _raise_for_pair(rc, bad, ctx)
    return gt[:n]


def pairings_product_gt(g1s, g2s) -> np.ndarray:
    """prod_k e(g1s[k], g2s[k]) as the host computes it (`kzg_pairings_product_gt`): (12, 4) uint64; the parity reference of
    `pairings_product_gt_batch`."""
    p1 = np.ascontiguousarray(_lib.as_u64(g1s, 8)).reshape(-1, 8)
    p2 = np.ascontiguousarray(_lib.as_u64(g2s, 16)).reshape(-1, 16)
    if len(p1) != len(p2):
        raise InvalidInputLength()
    gt = np.zeros((12, 4), dtype=np.uint64)
    rc = _lib.load().kzg_pairings_product_gt(_lib.ptr(p1) if len(p1) else None, _lib.ptr(p2) if len(p2) else None, len(p1), _lib.ptr(gt))
    if rc == _lib.ERR_G2_TAU_NOT_ON_CURVE:
        raise NotOnCurveError("G2 point not on curve")
    _raise_for(rc)
    return gt


def header_shifts(srs, srs_order: int, lens) -> dict:
    """{d: [tau^(srs_order - d)]_1 for d in lens}, read from a device-resident G1 SRS (`kzg_srs_download` of point srs_order - d): the
    `shifts` argument of verify_length_proof_batch.  d = srs_order gives the generator."""
    out = {}
    for d in sorted({int(d) for d in lens}):
        if d <= 0 or d > srs_order or srs_order - d >= len(srs):
            raise GenericError(f"the SRS of {len(srs)} points has no point tau^({srs_order} - {d})")
        pt = np.zeros(8, dtype=np.uint64)
        rc = _lib.load().kzg_srs_download(srs.ctx.handle, srs.handle, srs_order - d, 1, _lib.ptr(pt))
        _raise_for(rc, srs.ctx)
        out[d] = pt
    return out


def _header_args(commitments, length_commitments, length_proofs, claimed_lens, shifts):
    c = np.ascontiguousarray(_lib.as_u64(commitments, 8)).reshape(-1, 8)
    c2 = np.ascontiguousarray(_lib.as_u64(length_commitments, 16)).reshape(-1, 16)
    p2 = np.ascontiguousarray(_lib.as_u64(length_proofs, 16)).reshape(-1, 16)
    lens = np.ascontiguousarray([int(d) for d in claimed_lens], dtype=np.uint64)
    if not (len(c) == len(c2) == len(p2) == len(lens)):
        raise InvalidInputLength()
    shift_lens = np.ascontiguousarray([int(d) for d in shifts], dtype=np.uint64)
    shift_pts = np.ascontiguousarray([_lib.as_u64(shifts[d], 0).reshape(8) for d in shifts], dtype=np.uint64).reshape(-1, 8)
    return c, c2, p2, lens, shift_lens, shift_pts


def _opt(a):
    return _lib.ptr(a) if a.size else None


def compute_header_batch_weights(commitments, length_commitments, length_proofs, claimed_lens, shifts) -> np.ndarray:
    """The count + 1 weights (r_0 .. r_(count-1), rho) verify_length_proof_batch derives: (count + 1, 4) Fr wire words, each below 2^128
    (`kzg_compute_header_batch_weights`, host; the transcript is written out in the C header)."""
    c, c2, p2, lens, shift_lens, shift_pts = _header_args(commitments, length_commitments, length_proofs, claimed_lens, shifts)
    out = np.zeros((len(c) + 1, 4), dtype=np.uint64)
    rc = _lib.load().kzg_compute_header_batch_weights(_opt(c), _opt(c2), _opt(p2), _opt(lens), len(c), _opt(shift_lens), _opt(shift_pts), len(shift_lens),
                                                      _lib.ptr(out))
    _raise_for(rc)
    return out


def verify_length_proof_batch(commitments, length_commitments, length_proofs, claimed_lens, shifts, weights=None, ctx=None) -> bool:
    """`count` blob headers (C_i, C2_i, pi2_i, d_i) in ONE product of pairings (`kzg_verify_length_proof_batch`): the on-twist and
    order-r subgroup tests of both G2 elements and the weighted sums run on the GPU.  shifts = {d: [tau^(N-d)]_1} for every claimed
    length (header_shifts builds it from a G1 SRS); weights = None derives them from the transcript, else (count + 1, 4) Fr wire
    words r_0 .. r_(count-1), rho.  False = the equation failed (some header is bad: `locate_bad_headers` names it);
    NotOnCurveError names the first header with an input off its curve or outside the subgroup."""
    c, c2, p2, lens, shift_lens, shift_pts = _header_args(commitments, length_commitments, length_proofs, claimed_lens, shifts)
    w = _header_weights(weights, len(c))
    ctx = ctx or _lib.default_context()                             # (no context is created before the arguments pass)
    ok = _lib.i32(0)
    bad = C.c_uint64(0)
    rc = _lib.load().kzg_verify_length_proof_batch(ctx.handle, _opt(c), _opt(c2), _opt(p2), _opt(lens), len(c), _opt(shift_lens), _opt(shift_pts),
                                                   len(shift_lens), None if w is None else _lib.ptr(w), C.byref(ok), C.byref(bad))
    _raise_for_header(rc, bad, len(c), len(shift_lens), ctx)
    return bool(ok.value)


def _header_weights(weights, count):
    if weights is None:
        return None
    w = np.ascontiguousarray(_lib.as_u64(weights, 4)).reshape(-1, 4)
    if len(w) != count + 1:
        raise InvalidInputLength()
    return w


def _raise_for_header(rc, bad, count, n_shifts, ctx, grouped=False):
    """the statuses of the header-batch entries (kzg_verify_length_proof_batch and the two grouped entries behind it)"""
    if rc == _lib.ERR_G1_NOT_ON_CURVE:
        raise NotOnCurveError("G1 point %d not on curve" % bad.value)
    if rc == _lib.ERR_G2_TAU_NOT_ON_CURVE:
        raise NotOnCurveError("G2 point of header %d not on curve" % bad.value)
    if rc == _lib.ERR_NOT_ON_CURVE:
        raise NotOnCurveError("G2 point of header %d not in correct subgroup" % bad.value)
    if rc == _lib.ERR_NOT_POWER_OF_TWO:
        raise GenericError("a claimed length is not a power of two")
    if rc == _lib.ERR_INVALID_ARG and count and n_shifts:
        raise GenericError("a claimed length has no shift, a shift length is listed twice, more than 64 shifts, " +
                           ("a group index is not below n_groups, " if grouped else "") + "or slot 0 is in flight")
    _raise_for(rc, ctx)


def _header_group_args(groups, n_groups, count):
    """(group index per header, n_groups) for `groups` = "item" (one group per header) or an integer array with `n_groups`"""
    if isinstance(groups, str) and groups != "item":
        raise GenericError('groups is "item" or an array of group indices')
    return _group_args(groups, n_groups, None, 0, count)


def header_group_sums(commitments, length_commitments, length_proofs, claimed_lens, shifts, weights=None, ctx=None, groups="item", n_groups=None):
    """The components of every group's own header equation (`kzg_header_group_sums`), one pass on the GPU: U_g = sum r_i C_i,
    W_(g,s) = sum over the group's headers of the s-th listed length of r_i C2_i, Pi_g = sum r_i pi2_i, with the weights of
    `verify_length_proof_batch`.  Group g is good iff e(U_g, G2) e(-G1, sum_s W_(g,s) + [rho]Pi_g) prod_s e([rho]T_s, W_(g,s)) = 1, and the
    sums over all groups are what `verify_length_proof_batch` checks.  `groups` as for `locate_bad_headers`.  Returns (u, u_is_infinity,
    w, pi): (n_groups, 8) G1 wire points with a bool array, (n_groups, len(shifts), 16) and (n_groups, 16) G2 wire points (the identity
    all zeros; the length classes in the order of `shifts`); an empty group gives identities."""
    c, c2, p2, lens, shift_lens, shift_pts = _header_args(commitments, length_commitments, length_proofs, claimed_lens, shifts)
    w = _header_weights(weights, len(c))
    gi, n_groups = _header_group_args(groups, n_groups, len(c))
    ctx = ctx or _lib.default_context()
    n_shifts = len(shift_lens)
    u, uinf = np.zeros((n_groups, 8), np.uint64), np.zeros(max(n_groups, 1), np.uint8)
    wg, pi = np.zeros((n_groups, n_shifts, 16), np.uint64), np.zeros((n_groups, 16), np.uint64)
    bad = C.c_uint64(0)
    rc = _lib.load().kzg_header_group_sums(ctx.handle, _opt(c), _opt(c2), _opt(p2), _opt(lens), len(c), _opt(shift_lens), _opt(shift_pts), n_shifts,
                                           None if w is None else _lib.ptr(w), _opt(gi), n_groups, _opt(u), uinf.ctypes.data_as(_lib.u8p), _opt(wg), _opt(pi),
                                           C.byref(bad))
    _raise_for_header(rc, bad, len(c), n_shifts, ctx, grouped=True)
    return u, uinf[:n_groups].astype(bool), wg, pi


def locate_bad_headers(commitments, length_commitments, length_proofs, claimed_lens, shifts, weights=None, ctx=None, groups="item", n_groups=None):
    """Which groups of a batch of blob headers are bad (`kzg_verify_length_proof_batch_locate`): the group sums once on the GPU, then a
    search of the tree of those sums on the host, one product of pairings per step and at most 1 + 2 b ceil(log2 n_groups) of them for b
    bad groups.  `groups` = "item" (one group per header) or an integer array of group indices with `n_groups`; the other arguments are
    those of `verify_length_proof_batch`.  Returns (good, pairing_checks): a bool array of length n_groups (True = good) and the number
    of pairing checks; all True is the accept of `verify_length_proof_batch`.  This call always pays for the group sums: a caller who
    expects good batches calls `verify_length_proof_batch` first and this only after a reject.  The verdicts are sound for derived
    weights (weights=None, or `compute_header_batch_weights`); bad groups can cancel inside a range under weights of the caller's own."""
    c, c2, p2, lens, shift_lens, shift_pts = _header_args(commitments, length_commitments, length_proofs, claimed_lens, shifts)
    w = _header_weights(weights, len(c))
    gi, n_groups = _header_group_args(groups, n_groups, len(c))
    ctx = ctx or _lib.default_context()
    good = np.zeros(max(n_groups, 1), np.uint8)
    n_bad, checks, bad = _lib.sz(0), _lib.sz(0), C.c_uint64(0)
    rc = _lib.load().kzg_verify_length_proof_batch_locate(ctx.handle, _opt(c), _opt(c2), _opt(p2), _opt(lens), len(c), _opt(shift_lens), _opt(shift_pts),
                                                          len(shift_lens), None if w is None else _lib.ptr(w), _opt(gi), n_groups,
                                                          good.ctypes.data_as(_lib.u8p), C.byref(n_bad), C.byref(checks), C.byref(bad))
    _raise_for_header(rc, bad, len(c), len(shift_lens), ctx, grouped=True)
    good = good[:n_groups].astype(bool)
    assert int(n_bad.value) == int((~good).sum())
    return good, int(checks.value)


# ---- blob headers in their serialized form -----------------------------------------------------------------------------------------
# Per header: the commitment as 32 gnark-compressed bytes, the length commitment and the length proof as 64 gnark-compressed bytes each
# (the identity 0x40 and zeros), the claimed length as an integer.
_HEADER_ARRAYS = ("commitment", "length commitment", "length proof", "shift")


def _header_u8(data, per):
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    if len(buf) % per != 0:
        raise InvalidInputLength()
    return buf


def _header_bytes_args(commitments_be, length_commitments_be, length_proofs_be, claimed_lens, shifts):
    c, c2, p2 = _header_u8(commitments_be, 32), _header_u8(length_commitments_be, 64), _header_u8(length_proofs_be, 64)
    lens = np.ascontiguousarray([int(d) for d in claimed_lens], dtype=np.uint64)
    count = len(lens)
    if not (len(c) == 32 * count and len(c2) == 64 * count and len(p2) == 64 * count):
        raise InvalidInputLength()
    shift_lens = np.ascontiguousarray([int(d) for d in shifts], dtype=np.uint64)
    shift_pts = np.ascontiguousarray([_lib.as_u64(shifts[d], 0).reshape(8) for d in shifts], dtype=np.uint64).reshape(-1, 8)
    u8 = lambda a: a.ctypes.data_as(_lib.u8p) if a.size else None                       # noqa: E731
    return (c, c2, p2), (u8(c), u8(c2), u8(p2)), lens, shift_lens, shift_pts


def _raise_for_header_bytes(rc, bad, arr, count, n_shifts, ctx, grouped=False):
    """the statuses of the header entries on serialized input: a refused element by the name of its array and its header"""
    name = _HEADER_ARRAYS[arr.value] if 0 <= arr.value < 4 else "element"
    if rc == _lib.ERR_DESERIALIZE:
        raise DeserializationError("%s %d: not a canonical encoding (flag bits, or a coordinate not below the modulus)" % (name, bad.value))
    if rc == _lib.ERR_NOT_ON_CURVE:
        raise NotOnCurveError("%s %d: no such point on the curve" % (name, bad.value) if arr.value == 0 else
                              "%s %d: no such point on the twist, or not in the order-r subgroup" % (name, bad.value))
    if rc == _lib.ERR_G1_NOT_ON_CURVE:
        raise NotOnCurveError("shift %d not on curve" % bad.value)
    _raise_for_header(rc, bad, count, n_shifts, ctx, grouped)


def encode_header_items(commitments, length_commitments, length_proofs):
    """The disperser's half (`kzg_header_items_encode_be`, host): wire commitments (count, 8) and wire G2 elements (count, 16) each ->
    (commitments_be, length_commitments_be, length_proofs_be) bytes, 32 / 64 / 64 per header; an all-zero wire point encodes as the
    identity.  Any of the three may be None (its output is then None)."""
    arrs = [None if a is None else np.ascontiguousarray(_lib.as_u64(a, w)).reshape(-1, w) for a, w in ((commitments, 8), (length_commitments, 16), (length_proofs, 16))]
    counts = {len(a) for a in arrs if a is not None}
    if len(counts) > 1:
        raise InvalidInputLength()
    count = counts.pop() if counts else 0
    outs = [None if a is None else np.zeros(max(count * per, 1), np.uint8) for a, per in zip(arrs, (32, 64, 64))]
    if count:
        rc = _lib.load().kzg_header_items_encode_be(*[None if a is None else _lib.ptr(a) for a in arrs], count,
                                                    *[None if o is None else o.ctypes.data_as(_lib.u8p) for o in outs])
        if rc != _lib.OK:
            raise GenericError("a coordinate is not below the modulus" if rc == _lib.ERR_INVALID_ARG else _lib.status_message(rc))
    return tuple(None if o is None else o[:count * per].tobytes() for o, per in zip(outs, (32, 64, 64)))


def decode_header_items(commitments_be, length_commitments_be, length_proofs_be, ctx=None):
    """Serialized headers -> (commitments (count, 8), length_commitments (count, 16), length_proofs (count, 16)) wire words, decoded
    strictly on the GPU with the subgroup test of every G2 element (`kzg_header_items_decode_be`): what `verify_length_proof_batch`,
    `header_group_sums` and `locate_bad_headers` take.  DeserializationError / NotOnCurveError name the array and the header: a bad
    commitment first, then the smallest header with a bad G2 element, its length commitment in front of its length proof."""
    c, c2, p2 = _header_u8(commitments_be, 32), _header_u8(length_commitments_be, 64), _header_u8(length_proofs_be, 64)
    count = len(c) // 32
    if len(c2) != 64 * count or len(p2) != 64 * count:
        raise InvalidInputLength()
    out = np.zeros((count, 8), np.uint64), np.zeros((count, 16), np.uint64), np.zeros((count, 16), np.uint64)
    if count:
        ctx = ctx or _lib.default_context()
        bad, arr = C.c_uint64(0), _lib.i32(-1)
        rc = _lib.load().kzg_header_items_decode_be(ctx.handle, *[a.ctypes.data_as(_lib.u8p) for a in (c, c2, p2)], count, *[_lib.ptr(o) for o in out],
                                                    C.byref(bad), C.byref(arr))
        _raise_for_header_bytes(rc, bad, arr, count, 1, ctx)
    return out


def verify_length_proof_batch_bytes(commitments_be, length_commitments_be, length_proofs_be, claimed_lens, shifts, weights=None, ctx=None,
                                    return_weights=False):
    """`verify_length_proof_batch` on serialized headers, the decode inside the call (`kzg_verify_length_proof_batch_bytes`): one pass on
    the GPU decodes the G2 elements where the chains read them and runs their one subgroup test, the commitments are decoded into the
    bases of the G1 MSM, derived weights hash the items on the GPU.  The verdict and the weights are those of the decoded entry on
    `decode_header_items` of the same bytes.  DeserializationError / NotOnCurveError name the array and the header as
    `decode_header_items` does.  `return_weights=True` returns (ok, the count + 1 weights used)."""
    arrs, ptrs, lens, shift_lens, shift_pts = _header_bytes_args(commitments_be, length_commitments_be, length_proofs_be, claimed_lens, shifts)
    count = len(lens)
    w = _header_weights(weights, count)
    ctx = ctx or _lib.default_context()
    out_w = np.zeros((count + 1, 4), np.uint64)
    ok, bad, arr = _lib.i32(0), C.c_uint64(0), _lib.i32(-1)
    rc = _lib.load().kzg_verify_length_proof_batch_bytes(ctx.handle, *ptrs, _opt(lens), count, _opt(shift_lens), _opt(shift_pts), len(shift_lens),
                                                         None if w is None else _lib.ptr(w), C.byref(ok), _lib.ptr(out_w) if count else None, C.byref(bad),
                                                         C.byref(arr))
    _raise_for_header_bytes(rc, bad, arr, count, len(shift_lens), ctx)
    if count == 0 and return_weights:
        out_w = compute_header_batch_weights(np.zeros((0, 8), np.uint64), np.zeros((0, 16), np.uint64), np.zeros((0, 16), np.uint64), [], shifts) if w is None else w
    return (bool(ok.value), out_w) if return_weights else bool(ok.value)


def locate_bad_headers_bytes(commitments_be, length_commitments_be, length_proofs_be, claimed_lens, shifts, weights=None, ctx=None, groups="item",
                             n_groups=None):
    """`locate_bad_headers` on serialized headers (`kzg_verify_length_proof_batch_locate_bytes`): the prefix of
    `verify_length_proof_batch_bytes`, then the group sums and the search of the decoded entry.  Returns (good, pairing_checks), those of
    `locate_bad_headers` on `decode_header_items` of the same bytes."""
    arrs, ptrs, lens, shift_lens, shift_pts = _header_bytes_args(commitments_be, length_commitments_be, length_proofs_be, claimed_lens, shifts)
    count = len(lens)
    w = _header_weights(weights, count)
    gi, n_groups = _header_group_args(groups, n_groups, count)
    ctx = ctx or _lib.default_context()
    good = np.zeros(max(n_groups, 1), np.uint8)
    n_bad, checks, bad, arr = _lib.sz(0), _lib.sz(0), C.c_uint64(0), _lib.i32(-1)
    rc = _lib.load().kzg_verify_length_proof_batch_locate_bytes(ctx.handle, *ptrs, _opt(lens), count, _opt(shift_lens), _opt(shift_pts), len(shift_lens),
                                                                None if w is None else _lib.ptr(w), _opt(gi), n_groups, good.ctypes.data_as(_lib.u8p),
                                                                C.byref(n_bad), C.byref(checks), C.byref(bad), C.byref(arr))
    _raise_for_header_bytes(rc, bad, arr, count, len(shift_lens), ctx, grouped=True)
    good = good[:n_groups].astype(bool)
    assert int(n_bad.value) == int((~good).sum())
    return good, int(checks.value)


def verify_blob_kzg_proof(blob, commitment, proof, g2_tau=None, ctx=None) -> bool:
    """verify.rs:76-98 as ONE call of the C-ABI (`kzg_verify_blob_kzg_proof`)."""
    ctx = ctx or _lib.default_context()
    data = np.frombuffer(bytes(blob.data()), dtype=np.uint8) if len(blob.data()) else np.zeros(1, np.uint8)
    ok = _lib.i32(0)
    tau = None if g2_tau is None else _lib.as_u64(g2_tau, 0).reshape(16)
    rc = _lib.load().kzg_verify_blob_kzg_proof(ctx.handle, data.ctypes.data_as(_lib.u8p), len(blob.data()),
                                               _lib.ptr(_lib.as_u64(commitment, 0).reshape(8)), _lib.ptr(_lib.as_u64(proof, 0).reshape(8)),
                                               None if tau is None else _lib.ptr(tau), C.byref(ok))
    ctx.check_device(rc)
    _raise_for(rc)
    return bool(ok.value)


def verify_blob_kzg_proof_composed(blob, commitment, proof, g2_tau=None, ctx=None) -> bool:
    """verify.rs:76-98 composed from the reference's own steps (three calls); the one-call form above must agree with it."""
    helpers.validate_g1_point(commitment)
    helpers.validate_g1_point(proof)
    polynomial = blob.to_polynomial_eval_form()
    z = helpers.compute_challenge(blob, commitment)
    y = helpers.evaluate_polynomial_in_evaluation_form(polynomial, z, ctx)
    return verify_proof(commitment, proof, y, z, g2_tau)


def _pack(items, cols):
    n = len(items)
    return np.ascontiguousarray(np.stack([_lib.as_u64(x, 0).reshape(cols) for x in items])) if n else np.zeros((0, cols), np.uint64)


def compute_r_powers(commitments, zs, ys, proofs, blobs_as_field_elements_length) -> np.ndarray:
    """batch.rs:76-168 (`kzg_compute_r_powers`): r = H(domain || 0^8 || u64be(n) || n x u64be(len_i) || n x (C_i || z_i || y_i || proof_i)),
    returns [r^0 .. r^(n-1)]."""
    n = len(commitments)
    if n == 0:
        return np.zeros((0, 4), dtype=np.uint64)
    if not (len(zs) >= n and len(ys) >= n and len(proofs) >= n and len(blobs_as_field_elements_length) >= n):
        raise InvalidInputLength()
    cm, pf, z_, y_ = _pack(commitments, 8), _pack(proofs[:n], 8), _pack(zs[:n], 4), _pack(ys[:n], 4)
    lens = np.ascontiguousarray([int(v) for v in blobs_as_field_elements_length[:n]], dtype=np.uint64)
    out = np.zeros((n, 4), dtype=np.uint64)
    rc = _lib.load().kzg_compute_r_powers(_lib.ptr(cm), _lib.ptr(z_), _lib.ptr(y_), _lib.ptr(pf), _lib.ptr(lens), n, _lib.ptr(out))
    if rc != _lib.OK:
        raise GenericError(_lib.status_message(rc))
    return out


def compute_r_powers_py(commitments, zs, ys, proofs, blobs_as_field_elements_length) -> np.ndarray:
    """The same transcript assembled in Python (hashlib): an independent cross-check of the C path."""
    n = len(commitments)
    head = bytearray(40)
    head[0:24] = RANDOM_CHALLENGE_KZG_BATCH_DOMAIN
    head[32:40] = helpers.usize_to_be_bytes(n)
    parts = [bytes(head)] + [int(length).to_bytes(8, "big") for length in blobs_as_field_elements_length[:n]]
    for i in range(n):
        parts.append(helpers.serialize_compressed(commitments[i]))
        parts.append(fr_to_int(zs[i]).to_bytes(BYTES_PER_FIELD_ELEMENT, "big"))
        parts.append(fr_to_int(ys[i]).to_bytes(BYTES_PER_FIELD_ELEMENT, "big"))
        parts.append(helpers.serialize_compressed(proofs[i]))
    data = b"".join(parts)
    if len(data) != 40 + n * (4 * BYTES_PER_FIELD_ELEMENT + 8):
        raise InvalidInputLength()
    return helpers.compute_powers(helpers.hash_to_field_element(data), n)


def verify_kzg_proof_batch(commitments, zs, ys, proofs, blobs_as_field_elements_length, g2_tau=None, ctx=None) -> bool:
    """batch.rs:185-256."""
    if not (len(commitments) == len(zs) == len(ys) == len(proofs)):
        raise GenericError("length's of the input are not the same")
    for c in commitments:
        helpers.validate_g1_point(c)
    for p in proofs:
        helpers.validate_g1_point(p)
    ctx = ctx or _lib.default_context()
    n = len(commitments)
    r_powers = compute_r_powers(commitments, zs, ys, proofs, blobs_as_field_elements_length)

    cm, pf, z_, y_ = _pack(commitments, 8), _pack(proofs, 8), _pack(zs, 4), _pack(ys, 4)
    rp = np.ascontiguousarray(_lib.as_u64(r_powers, 4).reshape(-1, 4))
    tau = None if g2_tau is None else _lib.as_u64(g2_tau, 0).reshape(16)
    ok = _lib.i32(0)
    nul = None
    rc = _lib.load().kzg_verify_kzg_proof_batch(ctx.handle, _lib.ptr(cm) if n else nul, _lib.ptr(z_) if n else nul, _lib.ptr(y_) if n else nul,
                                                _lib.ptr(pf) if n else nul, _lib.ptr(rp) if n else nul, n,
                                                None if tau is None else _lib.ptr(tau), C.byref(ok))
    _raise_for(rc, ctx)
    return bool(ok.value)


def verify_blob_kzg_proof_batch(blobs, commitments, proofs, g2_tau=None, ctx=None) -> bool:
    """batch.rs:16-69 as ONE call of the C-ABI (`kzg_verify_blob_kzg_proof_batch`): point validation, the n Fiat-Shamir challenges
    (host thread pool), the n barycentric evaluations (one batched GPU launch), compute_r_powers, three batched GPU MSMs and the
    host 2-pairing check."""
    if not (len(commitments) == len(blobs) and len(proofs) == len(blobs)):
        raise GenericError("length's of the input are not the same")
    ctx = ctx or _lib.default_context()
    n = len(blobs)
    ptrs, lens, _keep = _lib.blob_args(blobs)
    cm, pf = _pack(commitments, 8), _pack(proofs, 8)
    tau = None if g2_tau is None else _lib.as_u64(g2_tau, 0).reshape(16)
    ok = _lib.i32(0)
    rc = _lib.load().kzg_verify_blob_kzg_proof_batch(ctx.handle, ptrs if n else None, lens if n else None, _lib.ptr(cm) if n else None,
                                                     _lib.ptr(pf) if n else None, n, None if tau is None else _lib.ptr(tau), C.byref(ok))
    _raise_for(rc, ctx)
    return bool(ok.value)


def verify_blob_kzg_proof_batch_py(blobs, commitments, proofs, g2_tau=None, ctx=None) -> bool:
    """The same flow step by step through the separate entry points (cross-check of the one-call form)."""
    if not (len(commitments) == len(blobs) and len(proofs) == len(blobs)):
        raise GenericError("length's of the input are not the same")
    for c in commitments:
        helpers.validate_g1_point(c)
    for p in proofs:
        helpers.validate_g1_point(p)
    zs, ys = helpers.compute_challenges_and_evaluate_polynomial(blobs, commitments, ctx)
    lengths = [len(b.to_polynomial_eval_form()) for b in blobs]
    return verify_kzg_proof_batch(commitments, zs, ys, proofs, lengths, g2_tau, ctx)


# ---- coset proofs (the proofs of KZG.compute_multiproofs; the reference has none) -------------------------------------------
COSET_ITEM_DOMAIN = b"KZGBN254_COSETITEM___V1_"
COSET_BATCH_DOMAIN = b"KZGBN254_COSETBATCH__V1_"


def _multiproof_args(commitments, commitment_indices, coset_indices, ys, proofs):
    ys = np.ascontiguousarray(_lib.as_u64(ys, 0))
    if ys.ndim != 3 or ys.shape[2] != 4:
        raise InvalidInputLength()
    count = ys.shape[0]
    cm, pf = _pack(commitments, 8), _pack(proofs, 8)
    ci = np.ascontiguousarray([int(v) for v in commitment_indices], dtype=np.uint64)
    ki = np.ascontiguousarray([int(v) for v in coset_indices], dtype=np.uint64)
    if not (len(pf) == len(ci) == len(ki) == count):
        raise GenericError("length's of the input are not the same")
    return cm, ci, ki, ys, pf


def compute_multiproof_r_powers(commitments, commitment_indices, coset_indices, ys, proofs, n: int, ctx=None, device=False) -> np.ndarray:
    """The weights [r^0 .. r^(count-1)] of a batch of coset proofs (`kzg_compute_multiproof_r_powers`, host only): item digests
    d_i = SHA-256(COSET_ITEM_DOMAIN || u64be(c_i) || u64be(k_i) || l x be32(ys_i[j]) || compressed proof_i), then
    r = SHA-256(COSET_BATCH_DOMAIN || u64be(n) || u64be(l) || u64be(M) || u64be(count) || M x compressed C || d_0 || ..) mod r.
    `device=True` hashes the item digests on the GPU of `ctx` (`kzg_compute_multiproof_r_powers_device`): the same bits."""
    cm, ci, ki, ys, pf = _multiproof_args(commitments, commitment_indices, coset_indices, ys, proofs)
    count, l = ys.shape[0], ys.shape[1]
    out = np.zeros((count, 4), dtype=np.uint64)
    if count == 0:
        return out
    args = (_lib.ptr(cm) if len(cm) else None, len(cm), _lib.ptr(ci), _lib.ptr(ki), _lib.ptr(ys), _lib.ptr(pf), count, int(n), l, _lib.ptr(out))
    if device:
        ctx = ctx or _lib.default_context()
        _raise_for(_lib.load().kzg_compute_multiproof_r_powers_device(ctx.handle, *args), ctx)
        return out
    rc = _lib.load().kzg_compute_multiproof_r_powers(*args)
    if rc != _lib.OK:
        raise GenericError(_lib.status_message(rc))
    return out


def compute_multiproof_r_powers_py(commitments, commitment_indices, coset_indices, ys, proofs, n: int) -> np.ndarray:
    """The same transcript assembled in Python (hashlib): an independent cross-check of the C path."""
    ys = np.asarray(ys, dtype=np.uint64)
    count, l = ys.shape[0], ys.shape[1]
    parts = [COSET_BATCH_DOMAIN, int(n).to_bytes(8, "big"), int(l).to_bytes(8, "big"), len(commitments).to_bytes(8, "big"),
             int(count).to_bytes(8, "big")]
    parts += [helpers.serialize_compressed(c) for c in commitments]
    for i in range(count):
        item = COSET_ITEM_DOMAIN + int(commitment_indices[i]).to_bytes(8, "big") + int(coset_indices[i]).to_bytes(8, "big")
        item += b"".join(fr_to_int(ys[i, j]).to_bytes(BYTES_PER_FIELD_ELEMENT, "big") for j in range(l))
        item += helpers.serialize_compressed(proofs[i])
        parts.append(hashlib.sha256(item).digest())
    return helpers.compute_powers(helpers.hash_to_field_element(b"".join(parts)), count)


def verify_multiproof_batch(commitments, commitment_indices, coset_indices, ys, proofs, n: int, srs, g2_tau_l=None, r_powers=None,
                            ctx=None) -> bool:
    """A batch of coset proofs in ONE pairing check (`kzg_verify_multiproof_batch`).  Item i: commitment `commitments[commitment_indices[i]]`,
    coset `coset_indices[i]` of the n-point domain, its l values `ys[i]` (= evals[k::n // l], `KZG.cosets`) and `proofs[i]` (row k of
    `KZG.compute_multiproofs`).  `srs` needs its first l points only; `g2_tau_l` = [tau^l]_2 (G2 wire point; None is allowed for l = 1
    and means consts::G2_TAU); `r_powers=None` derives the weights with `compute_multiproof_r_powers`."""
    cm, ci, ki, ys, pf = _multiproof_args(commitments, commitment_indices, coset_indices, ys, proofs)
    count, l = ys.shape[0], ys.shape[1]
    if g2_tau_l is None and l != 1:
        raise GenericError("g2_tau_l = None (consts::G2_TAU) is [tau]_2: chunks of more than one point need [tau^l]_2")
    ctx = ctx or getattr(srs, "ctx", None) or _lib.default_context()                   # the SRS's own context
    rp = None if r_powers is None else np.ascontiguousarray(_lib.as_u64(r_powers, 0)).reshape(-1, 4)
    if rp is not None and len(rp) != count:
        raise GenericError("length's of the input are not the same")
    ok = _lib.i32(0)
    rc = _lib.load().kzg_verify_multiproof_batch(ctx.handle, srs.handle, _lib.ptr(cm) if len(cm) else None, len(cm),
                                                 _lib.ptr(ci) if count else None, _lib.ptr(ki) if count else None,
                                                 _lib.ptr(ys) if count else None, _lib.ptr(pf) if count else None, count, int(n), l,
                                                 None if rp is None or count == 0 else _lib.ptr(rp), _g2_arg(g2_tau_l), C.byref(ok))
    _raise_for(rc, ctx)
    return bool(ok.value)


def verify_multiproof(commitment, proof, coset_index: int, ys, n: int, srs, g2_tau_l=None, ctx=None) -> bool:
    """One coset proof (`kzg_verify_multiproof`): e(proof, [tau^l]_2 - [w^(k l)]G2) = e(C - [I_k(tau)]_1, G2) with I_k the polynomial
    through the l values `ys` on coset `coset_index`.  For l = 1 this is `verify_proof(commitment, proof, ys[0], w^k)`."""
    ys = np.ascontiguousarray(_lib.as_u64(ys, 0)).reshape(-1, 4)
    if g2_tau_l is None and len(ys) != 1:
        raise GenericError("g2_tau_l = None (consts::G2_TAU) is [tau]_2: chunks of more than one point need [tau^l]_2")
    ctx = ctx or getattr(srs, "ctx", None) or _lib.default_context()
    ok = _lib.i32(0)
    rc = _lib.load().kzg_verify_multiproof(ctx.handle, srs.handle, _lib.ptr(_lib.as_u64(commitment, 0).reshape(8)),
                                           _lib.ptr(_lib.as_u64(proof, 0).reshape(8)), int(coset_index), _lib.ptr(ys), int(n), len(ys),
                                           _g2_arg(g2_tau_l), C.byref(ok))
    _raise_for(rc, ctx)
    return bool(ok.value)


# ---- coset proofs of MIXED blob shapes in one call ----------------------------------------------------------------------------------
COSET_MIXED_DOMAIN = b"KZGBN254_COSETMIXED__V1_"


def _mixed_args(classes, class_indices, coset_indices, ys):
    """classes: a sequence of (n, l); ys: a sequence of (l_i, 4) arrays, or one flat (sum l_i, 4) array -> the class tables, the index arrays
    and the ragged values as one contiguous (sum l_i, 4) array."""
    cn = np.ascontiguousarray([int(c[0]) for c in classes], dtype=np.uint64)
    cl = np.ascontiguousarray([int(c[1]) for c in classes], dtype=np.uint64)
    si = np.ascontiguousarray([int(v) for v in class_indices], dtype=np.uint64)
    ki = np.ascontiguousarray([int(v) for v in coset_indices], dtype=np.uint64)
    if len(si) != len(ki):
        raise GenericError("length's of the input are not the same")
    if isinstance(ys, np.ndarray) and ys.ndim == 2:
        flat = np.ascontiguousarray(_lib.as_u64(ys, 0))
    else:
        rows = [np.ascontiguousarray(_lib.as_u64(y, 0)).reshape(-1, 4) for y in ys]
        if len(rows) != len(si):
            raise GenericError("length's of the input are not the same")
        for s, row in zip(si, rows):
            if int(s) < len(cl) and len(row) != int(cl[int(s)]):
                raise InvalidInputLength()
        flat = np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros((0, 4), np.uint64)
    if flat.ndim != 2 or flat.shape[1] != 4:
        raise InvalidInputLength()
    if all(int(s) < len(cl) for s in si) and len(flat) != sum(int(cl[int(s)]) for s in si):
        raise InvalidInputLength()
    return cn, cl, si, ki, flat


def _opt(a):
    return _lib.ptr(a) if len(a) else None


def compute_multiproof_r_powers_mixed(commitments, commitment_indices, classes, class_indices, coset_indices, ys, proofs) -> np.ndarray:
    """The weights [r^0 .. r^(count-1)] of a batch of coset proofs of mixed shapes (`kzg_compute_multiproof_r_powers_mixed`, host only): the
    item digests of `compute_multiproof_r_powers` over each item's own l values, then r = SHA-256(COSET_MIXED_DOMAIN || u64be(n_classes) ||
    n_classes x (u64be(n_s) || u64be(l_s)) || u64be(M) || u64be(count) || count x u64be(s_i) || M x compressed C || d_0 || ..) mod r."""
    cn, cl, si, ki, flat = _mixed_args(classes, class_indices, coset_indices, ys)
    cm, pf = _pack(commitments, 8), _pack(proofs, 8)
    ci = np.ascontiguousarray([int(v) for v in commitment_indices], dtype=np.uint64)
    count = len(si)
    if not (len(pf) == len(ci) == count):
        raise GenericError("length's of the input are not the same")
    out = np.zeros((count, 4), dtype=np.uint64)
    if count == 0:
        return out
    rc = _lib.load().kzg_compute_multiproof_r_powers_mixed(_opt(cm), len(cm), _lib.ptr(ci), _opt(cn), _opt(cl), len(cn), _lib.ptr(si), _lib.ptr(ki),
                                                           _opt(flat), _lib.ptr(pf), count, _lib.ptr(out))
    if rc != _lib.OK:
        raise GenericError(_lib.status_message(rc))
    return out


def verify_multiproof_batch_mixed(commitments, commitment_indices, classes, class_indices, coset_indices, ys, proofs, srs, g2_tau_l, r_powers=None,
                                  ctx=None) -> bool:
    """A batch of coset proofs of MIXED blob shapes in one call and ONE product of pairings (`kzg_verify_multiproof_batch_mixed`).  `classes` is a
    sequence of (n, l); item i has the class `class_indices[i]`, the commitment `commitments[commitment_indices[i]]`, the coset `coset_indices[i]`
    of its class's domain, its l values `ys[i]` and `proofs[i]`.  `ys` is a sequence of (l_i, 4) arrays or one flat (sum l_i, 4) array in item
    order.  `g2_tau_l` has one G2 point per class, entry s = [tau^(l_s)]_2 (never None).  `srs` needs its first max(l_s) points.  The product has
    1 + (distinct chunk lengths) pairs whatever the item count.  `r_powers=None` derives the weights with `compute_multiproof_r_powers_mixed`
    (on the host: this entry has no device transcript).  Measured against one `verify_multiproof_batch` call per class
    (profiles/multiproof_verify_mixed.md): 64 blobs x 64 chunks over 8 classes 2.46 ms against 15.7 ms; two classes of 32 768 items each 13.5 ms
    against 8.7 ms -- SLOWER than the loop, whose large classes are hashed on the device (equal, 13.5 against 14.0 ms, with the loop's digests on the
    host); one class of 65 536 x 64 17.1 ms against 7.8 ms.  A batch of ONE shape, or of few large classes, belongs to `verify_multiproof_batch`."""
    cn, cl, si, ki, flat = _mixed_args(classes, class_indices, coset_indices, ys)
    cm, pf = _pack(commitments, 8), _pack(proofs, 8)
    ci = np.ascontiguousarray([int(v) for v in commitment_indices], dtype=np.uint64)
    count = len(si)
    if not (len(pf) == len(ci) == count):
        raise GenericError("length's of the input are not the same")
    g2 = np.ascontiguousarray(np.stack([_lib.as_u64(p, 0).reshape(16) for p in g2_tau_l])) if len(g2_tau_l) else np.zeros((0, 16), np.uint64)
    if len(g2) != len(cn):
        raise GenericError("g2_tau_l needs one point per class")
    ctx = ctx or getattr(srs, "ctx", None) or _lib.default_context()                   # the SRS's own context
    rp = None if r_powers is None else np.ascontiguousarray(_lib.as_u64(r_powers, 0)).reshape(-1, 4)
    if rp is not None and len(rp) != count:
        raise GenericError("length's of the input are not the same")
    ok = _lib.i32(0)
    rc = _lib.load().kzg_verify_multiproof_batch_mixed(ctx.handle, srs.handle, _opt(cm), len(cm), _opt(ci), _opt(cn), _opt(cl), len(cn), _opt(si), _opt(ki),
                                                       _opt(flat), _opt(pf), count, None if rp is None or count == 0 else _lib.ptr(rp), _opt(g2), C.byref(ok))
    _raise_for(rc, ctx)
    return bool(ok.value)


# ---- coset items in their serialized form ------------------------------------------------------------------------------------------
# A commitment or proof is a 32-byte gnark-compressed G1 point, a value a 32-byte big-endian scalar.
_ARRAYS = ("commitment", "proof", "value of item")


def _u8_arg(data, want_len, what):
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    if len(buf) != want_len:
        raise InvalidInputLength()
    return buf, (buf.ctypes.data_as(_lib.u8p) if len(buf) else None)


def encode_coset_items(ys, proofs):
    """The disperser's half (`kzg_coset_items_encode_be`, host): values (count, l, 4) and wire proofs (count, 8) -> (ys_be, proofs_be)
    bytes, 32 per value and per proof.  Either may be None."""
    ys_a = None if ys is None else np.ascontiguousarray(_lib.as_u64(ys, 0))
    if ys_a is not None and (ys_a.ndim != 3 or ys_a.shape[2] != 4):
        raise InvalidInputLength()
    pf = None if proofs is None else _pack(proofs, 8)
    count = len(ys_a) if ys_a is not None else len(pf) if pf is not None else 0
    if ys_a is not None and pf is not None and len(pf) != count:
        raise GenericError("length's of the input are not the same")
    l = ys_a.shape[1] if ys_a is not None else 1
    out_y = np.zeros(max(count * l * 32, 1), np.uint8) if ys_a is not None else None
    out_p = np.zeros(max(count * 32, 1), np.uint8) if pf is not None else None
    if count:
        rc = _lib.load().kzg_coset_items_encode_be(None if ys_a is None else _lib.ptr(ys_a), None if pf is None else _lib.ptr(pf), count, l,
                                                   None if out_y is None else out_y.ctypes.data_as(_lib.u8p),
                                                   None if out_p is None else out_p.ctypes.data_as(_lib.u8p))
        if rc != _lib.OK:
            raise GenericError("a value or coordinate is not below its modulus" if rc == _lib.ERR_INVALID_ARG else _lib.status_message(rc))
    return (None if out_y is None else out_y[:count * l * 32].tobytes()), (None if out_p is None else out_p[:count * 32].tobytes())


def decode_coset_items(ys_be, proofs_be, chunk_len: int, ctx=None):
    """Serialized items -> (ys (count, l, 4), proofs (count, 8)) wire words, decoded strictly on the GPU (`kzg_coset_items_decode_be`):
    what `locate_bad_multiproofs`, `coset_group_sums` and `KZG.recover_from_cosets` take.  Either input may be None (its output is then
    None).  DeserializationError / NotOnCurveError name the array and the item; proofs are checked before values."""
    l = int(chunk_len)
    if ys_be is None and proofs_be is None:
        raise InvalidInputLength()
    if ys_be is not None and (l <= 0 or len(ys_be) % (32 * l) != 0) or proofs_be is not None and len(proofs_be) % 32 != 0:
        raise InvalidInputLength()
    count = len(ys_be) // (32 * l) if ys_be is not None else len(proofs_be) // 32
    yb, yp = (None, None) if ys_be is None else _u8_arg(ys_be, count * l * 32, "values")
    pb, pp = (None, None) if proofs_be is None else _u8_arg(proofs_be, count * 32, "proofs")
    ctx = ctx or _lib.default_context()
    ys = None if ys_be is None else np.zeros((count, l, 4), np.uint64)
    pf = None if proofs_be is None else np.zeros((count, 8), np.uint64)
    if count:
        bad, arr = C.c_uint64(0), _lib.i32(0)
        rc = _lib.load().kzg_coset_items_decode_be(ctx.handle, yp, pp, count, l, None if ys is None else _lib.ptr(ys), None if pf is None else _lib.ptr(pf),
                                                   C.byref(bad), C.byref(arr))
        helpers.raise_for_decode(rc, _ARRAYS[arr.value] if 0 <= arr.value < 3 else "element", bad.value, ctx)
    return ys, pf


def _bytes_args(commitments_be, commitment_indices, coset_indices, ys_be, proofs_be, chunk_len):
    l = int(chunk_len)
    if l <= 0 or len(proofs_be) % 32 != 0 or len(commitments_be) % 32 != 0:
        raise InvalidInputLength()
    count = len(proofs_be) // 32
    ci = np.ascontiguousarray([int(v) for v in commitment_indices], dtype=np.uint64)
    ki = np.ascontiguousarray([int(v) for v in coset_indices], dtype=np.uint64)
    if not (len(ci) == len(ki) == count):
        raise GenericError("length's of the input are not the same")
    cm = _u8_arg(commitments_be, len(commitments_be), "commitments")
    ys = _u8_arg(ys_be, count * l * 32, "values")
    pf = _u8_arg(proofs_be, count * 32, "proofs")
    return cm, ci, ki, ys, pf, count, l


def compute_multiproof_r_powers_bytes(commitments_be, commitment_indices, coset_indices, ys_be, proofs_be, n: int, chunk_len: int) -> np.ndarray:
    """The weights of `compute_multiproof_r_powers`, bit for bit, from the serialized form of the same items
    (`kzg_compute_multiproof_r_powers_bytes`, host only): the item message is assembled from the bytes, no field arithmetic before the
    final mod r.  Bytes that do not decode are hashed as given."""
    cm, ci, ki, ys, pf, count, l = _bytes_args(commitments_be, commitment_indices, coset_indices, ys_be, proofs_be, chunk_len)
    out = np.zeros((count, 4), dtype=np.uint64)
    if count:
        rc = _lib.load().kzg_compute_multiproof_r_powers_bytes(cm[1], len(cm[0]) // 32, _lib.ptr(ci), _lib.ptr(ki), ys[1], pf[1], count, int(n), l, _lib.ptr(out))
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
    return out


def verify_multiproof_batch_bytes(commitments_be, commitment_indices, coset_indices, ys_be, proofs_be, n: int, chunk_len: int, srs, g2_tau_l=None,
                                  r_powers=None, ctx=None, return_r_powers=False):
    """`verify_multiproof_batch` on serialized items, the decode inside the call (`kzg_verify_multiproof_batch_bytes`): commitments_be
    M x 32, proofs_be count x 32, ys_be count x l x 32 bytes.  The verdict and the weights are those of the decoded entry on the decoded
    inputs.  DeserializationError / NotOnCurveError name the array (commitment, proof, value of item) and the index, in that order of
    arrays.  `return_r_powers=True` returns (ok, weights used)."""
    cm, ci, ki, ys, pf, count, l = _bytes_args(commitments_be, commitment_indices, coset_indices, ys_be, proofs_be, chunk_len)
    if g2_tau_l is None and l != 1:
        raise GenericError("g2_tau_l = None (consts::G2_TAU) is [tau]_2: chunks of more than one point need [tau^l]_2")
    ctx = ctx or getattr(srs, "ctx", None) or _lib.default_context()
    rp = None if r_powers is None else np.ascontiguousarray(_lib.as_u64(r_powers, 0)).reshape(-1, 4)
    if rp is not None and len(rp) != count:
        raise GenericError("length's of the input are not the same")
    out_rp = np.zeros((count, 4), dtype=np.uint64)
    ok, bad, arr = _lib.i32(0), C.c_uint64(0), _lib.i32(-1)
    rc = _lib.load().kzg_verify_multiproof_batch_bytes(ctx.handle, srs.handle, cm[1], len(cm[0]) // 32, _lib.ptr(ci) if count else None,
                                                       _lib.ptr(ki) if count else None, ys[1], pf[1], count, int(n), l,
                                                       None if rp is None or count == 0 else _lib.ptr(rp), _g2_arg(g2_tau_l), C.byref(ok),
                                                       _lib.ptr(out_rp) if count else None, C.byref(bad), C.byref(arr))
    if rc in (_lib.ERR_DESERIALIZE, _lib.ERR_NOT_ON_CURVE):
        helpers.raise_for_decode(rc, _ARRAYS[arr.value] if 0 <= arr.value < 3 else "element", bad.value, ctx)
    _raise_for(rc, ctx)
    return (bool(ok.value), out_rp) if return_r_powers else bool(ok.value)


def retrieve_blobs_bytes(commitments_be, coset_indices, ys_be, proofs_be, n: int, chunk_len: int, srs, g2_tau_l=None, degree_bound=None,
                         eval_form: bool = True, out_len=None, r_powers=None, ctx=None):
    """The retriever's call (`kzg_retrieve_blobs_bytes`): verify the chunks of B blobs against their commitments and, if the batch is
    accepted, recover the blobs -- values uploaded once, bytes in and bytes out.  commitments_be B x 32 bytes; `coset_indices` (count,)
    or (B, count); ys_be B x count x l x 32 and proofs_be B x count x 32 bytes.  Returns (ok, polys_be, consistent): with ok True the
    outputs of `KZG.recover_from_cosets_batch_bytes`, with ok False (None, None) -- go to `locate_bad_multiproofs`.  The verdict, the
    weights and the refusals (DeserializationError / NotOnCurveError naming array and index) are those of `verify_multiproof_batch_bytes`
    on the B x count items."""
    n, l = int(n), int(chunk_len)
    idx = np.ascontiguousarray(coset_indices, dtype=np.uint64)
    if l <= 0 or len(commitments_be) == 0 or len(commitments_be) % 32 != 0 or idx.ndim not in (1, 2) or idx.shape[-1] == 0:
        raise InvalidInputLength()
    blobs, count = len(commitments_be) // 32, int(idx.shape[-1])
    if idx.ndim == 2 and idx.shape[0] != blobs:
        raise GenericError("coset indices must have the shape (count,) or (B, count)")
    if g2_tau_l is None and l != 1:
        raise GenericError("g2_tau_l = None (consts::G2_TAU) is [tau]_2: chunks of more than one point need [tau^l]_2")
    cm = _u8_arg(commitments_be, blobs * 32, "commitments")
    ys = _u8_arg(ys_be, blobs * count * l * 32, "values")
    pf = _u8_arg(proofs_be, blobs * count * 32, "proofs")
    rp = None if r_powers is None else np.ascontiguousarray(_lib.as_u64(r_powers, 0)).reshape(-1, 4)
    if rp is not None and len(rp) != blobs * count:
        raise GenericError("length's of the input are not the same")
    bound = 0 if not degree_bound else int(degree_bound)
    rows = n if not out_len else int(out_len)
    if rows <= 0 or bound < 0:
        raise GenericError("out_len is for coefficients, between the degree bound and n")
    ctx = ctx or getattr(srs, "ctx", None) or _lib.default_context()
    out = np.zeros(blobs * rows * 32, dtype=np.uint8)
    consistent = np.zeros(blobs, dtype=np.int32)
    ok, bad, arr = _lib.i32(0), C.c_uint64(0), _lib.i32(-1)
    rc = _lib.load().kzg_retrieve_blobs_bytes(ctx.handle, srs.handle, cm[1], _lib.ptr(idx), 1 if idx.ndim == 1 else blobs, ys[1], pf[1], blobs, count, n, l, bound,
                                              1 if eval_form else 0, rows, None if rp is None else _lib.ptr(rp), _g2_arg(g2_tau_l), C.byref(ok),
                                              out.ctypes.data_as(_lib.u8p), consistent.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(bad), C.byref(arr))
    if rc in (_lib.ERR_DESERIALIZE, _lib.ERR_NOT_ON_CURVE):
        helpers.raise_for_decode(rc, _ARRAYS[arr.value] if 0 <= arr.value < 3 else "element", bad.value, ctx)
    if rc == _lib.ERR_INVALID_ARG:
        raise GenericError("the shape, the coset indices (distinct, below n / chunk length), the degree bound or out_len is not valid, the SRS is not "
                           "this context's monomial one, or slot 0 is in flight")
    _raise_for(rc, ctx)
    if not ok.value:
        return False, None, None
    return True, out.tobytes(), consistent.astype(bool)


def retrieve_blobs_bytes_tolerant(commitments_be, coset_indices, ys_be, proofs_be, n: int, chunk_len: int, srs, use_count=None, g2_tau_l=None,
                                  degree_bound=None, eval_form: bool = True, out_len=None, r_powers=None, ctx=None, return_checks=False, return_r_powers=False):
    """The retriever's call that survives bad chunks (`kzg_retrieve_blobs_bytes_tolerant`): arguments as `retrieve_blobs_bytes`, a blob
    holding `count` chunks of which the first `use_count` (default: count) good ones, in item order, recover it.  Returns (item_status,
    blob_ok, polys_be, consistent): item_status (B, count) uint8 -- 0 good, 1 fails its equation, 2 proof bytes not canonical, 3 proof x
    off the curve, 4 a value >= r; blob_ok (B,) bool, False for a blob with fewer than use_count good items (its row is zero bytes and its
    flag False); polys_be and consistent as `KZG.recover_from_cosets_batch_bytes` gives them for the chosen chunks.  The batch equation runs
    once; only after a reject are the bad items located, on the device-resident items, blobs first and then the items of the bad blobs.
    A commitment that does not decode raises as in `retrieve_blobs_bytes`.  `return_checks=True` appends the number of pairing checks, `return_r_powers=True` the
    (B * count, 4) weights used (zero at every refused item)."""
    n, l = int(n), int(chunk_len)
    idx = np.ascontiguousarray(coset_indices, dtype=np.uint64)
    if l <= 0 or len(commitments_be) == 0 or len(commitments_be) % 32 != 0 or idx.ndim not in (1, 2) or idx.shape[-1] == 0:
        raise InvalidInputLength()
    blobs, count = len(commitments_be) // 32, int(idx.shape[-1])
    if idx.ndim == 2 and idx.shape[0] != blobs:
        raise GenericError("coset indices must have the shape (count,) or (B, count)")
    if g2_tau_l is None and l != 1:
        raise GenericError("g2_tau_l = None (consts::G2_TAU) is [tau]_2: chunks of more than one point need [tau^l]_2")
    use = count if use_count is None else int(use_count)
    cm = _u8_arg(commitments_be, blobs * 32, "commitments")
    ys = _u8_arg(ys_be, blobs * count * l * 32, "values")
    pf = _u8_arg(proofs_be, blobs * count * 32, "proofs")
    rp = None if r_powers is None else np.ascontiguousarray(_lib.as_u64(r_powers, 0)).reshape(-1, 4)
    if rp is not None and len(rp) != blobs * count:
        raise GenericError("length's of the input are not the same")
    bound = 0 if not degree_bound else int(degree_bound)
    rows = n if not out_len else int(out_len)
    if rows <= 0 or bound < 0 or use < 0:
        raise GenericError("out_len is for coefficients, between the degree bound and n")
    ctx = ctx or getattr(srs, "ctx", None) or _lib.default_context()
    out = np.zeros(blobs * rows * 32, dtype=np.uint8)
    consistent = np.zeros(blobs, dtype=np.int32)
    item_status = np.zeros(blobs * count, dtype=np.uint8)
    blob_status = np.zeros(blobs, dtype=np.uint8)
    bad_items, unrecovered, checks, bad, arr = _lib.sz(0), _lib.sz(0), _lib.sz(0), C.c_uint64(0), _lib.i32(-1)
    used = np.zeros((blobs * count, 4), dtype=np.uint64)
    rc = _lib.load().kzg_retrieve_blobs_bytes_tolerant(ctx.handle, srs.handle, cm[1], _lib.ptr(idx), 1 if idx.ndim == 1 else blobs, ys[1], pf[1], blobs, count, use, n, l,
                                                       bound, 1 if eval_form else 0, rows, None if rp is None else _lib.ptr(rp), _g2_arg(g2_tau_l),
                                                       item_status.ctypes.data_as(_lib.u8p), blob_status.ctypes.data_as(_lib.u8p), C.byref(bad_items),
                                                       C.byref(unrecovered), C.byref(checks), out.ctypes.data_as(_lib.u8p),
                                                       consistent.ctypes.data_as(C.POINTER(C.c_int32)), _lib.ptr(used), C.byref(bad), C.byref(arr))
    if rc in (_lib.ERR_DESERIALIZE, _lib.ERR_NOT_ON_CURVE):
        helpers.raise_for_decode(rc, _ARRAYS[arr.value] if 0 <= arr.value < 3 else "element", bad.value, ctx)
    if rc == _lib.ERR_INVALID_ARG:
        raise GenericError("the shape, use_count, the coset indices (distinct, below n / chunk length), the degree bound or out_len is not valid, the SRS is "
                           "not this context's monomial one, or slot 0 is in flight")
    _raise_for(rc, ctx)
    assert int(bad_items.value) == int((item_status != 0).sum()) and int(unrecovered.value) == int(blob_status.sum())
    res = (item_status.reshape(blobs, count), blob_status == 0, out.tobytes(), consistent.astype(bool))
    if return_checks:
        res += (int(checks.value),)
    return res + (used,) if return_r_powers else res


def locate_bad_multiproofs_bytes(commitments_be, commitment_indices, coset_indices, ys_be, proofs_be, n: int, chunk_len: int, srs, g2_tau_l=None,
                                 r_powers=None, ctx=None, groups="commitment", n_groups=None, return_r_powers=False):
    """`locate_bad_multiproofs` on serialized items, the decode inside the call (`kzg_verify_multiproof_batch_locate_bytes`): the items go
    up once as bytes and nothing decoded returns to the host.  Returns (good, pairing_checks), with `return_r_powers=True` also the weights
    used; they are those of `locate_bad_multiproofs` on the decoded items.  DeserializationError / NotOnCurveError as
    `verify_multiproof_batch_bytes` raises them."""
    cm, ci, ki, ys, pf, count, l = _bytes_args(commitments_be, commitment_indices, coset_indices, ys_be, proofs_be, chunk_len)
    if g2_tau_l is None and l != 1:
        raise GenericError("g2_tau_l = None (consts::G2_TAU) is [tau]_2: chunks of more than one point need [tau^l]_2")
    gi, n_groups = _group_args(groups, n_groups, ci, len(cm[0]) // 32, count)
    ctx = ctx or getattr(srs, "ctx", None) or _lib.default_context()
    rp = None if r_powers is None else np.ascontiguousarray(_lib.as_u64(r_powers, 0)).reshape(-1, 4)
    if rp is not None and len(rp) != count:
        raise GenericError("length's of the input are not the same")
    opt = lambda a: _lib.ptr(a) if count else None                                     # noqa: E731
    good = np.zeros(max(n_groups, 1), np.uint8)
    out_rp = np.zeros((count, 4), dtype=np.uint64)
    n_bad, checks, bad, arr = _lib.sz(0), _lib.sz(0), C.c_uint64(0), _lib.i32(-1)
    rc = _lib.load().kzg_verify_multiproof_batch_locate_bytes(ctx.handle, srs.handle, cm[1], len(cm[0]) // 32, opt(ci), opt(ki), ys[1], pf[1], count, int(n), l,
                                                              None if rp is None or count == 0 else _lib.ptr(rp), _g2_arg(g2_tau_l), opt(gi), n_groups,
                                                              good.ctypes.data_as(_lib.u8p), C.byref(n_bad), C.byref(checks), opt(out_rp), C.byref(bad),
                                                              C.byref(arr))
    if rc in (_lib.ERR_DESERIALIZE, _lib.ERR_NOT_ON_CURVE):
        helpers.raise_for_decode(rc, _ARRAYS[arr.value] if 0 <= arr.value < 3 else "element", bad.value, ctx)
    _raise_for(rc, ctx)
    good = good[:n_groups].astype(bool)
    assert int(n_bad.value) == int((~good).sum())
    return (good, int(checks.value), out_rp) if return_r_powers else (good, int(checks.value))


# ---- locating the bad items of a rejected batch ----------------------------------------------------------------------------------
pairings_verify = helpers.pairings_verify          # e(a1, a2) == e(b1, b2): the check of one pair of group sums against ([tau^l]_2, G2)


def _group_args(groups, n_groups, commitment_indices, n_commitments, count):
    """(group index per item, n_groups) for `groups` = "commitment" (group = commitment row), "item" (one group per item) or an explicit
    integer array with `n_groups`."""
    if isinstance(groups, str):
        if groups == "commitment":
            return np.ascontiguousarray(commitment_indices, dtype=np.uint64), int(n_commitments)
        if groups == "item":
            return np.arange(count, dtype=np.uint64), int(count)
        raise GenericError('groups is "commitment", "item" or an array of group indices')
    gi = np.ascontiguousarray([int(v) for v in groups], dtype=np.uint64)
    if len(gi) != count:
        raise GenericError("length's of the input are not the same")
    if n_groups is None:
        raise GenericError("an explicit grouping needs n_groups")
    return gi, int(n_groups)


def _locate_args(commitments, commitment_indices, coset_indices, ys, proofs, srs, g2_tau_l, r_powers, ctx, groups, n_groups, need_g2):
    cm, ci, ki, ys, pf = _multiproof_args(commitments, commitment_indices, coset_indices, ys, proofs)
    count, l = ys.shape[0], ys.shape[1]
    if need_g2 and g2_tau_l is None and l != 1:
        raise GenericError("g2_tau_l = None (consts::G2_TAU) is [tau]_2: chunks of more than one point need [tau^l]_2")
    gi, n_groups = _group_args(groups, n_groups, ci, len(cm), count)
    rp = None if r_powers is None else np.ascontiguousarray(_lib.as_u64(r_powers, 0)).reshape(-1, 4)
    if rp is not None and len(rp) != count:
        raise GenericError("length's of the input are not the same")
    ctx = ctx or getattr(srs, "ctx", None) or _lib.default_context()                   # the SRS's own context
    opt = lambda a: _lib.ptr(a) if count else None                                     # noqa: E731
    head = (ctx.handle, srs.handle, _lib.ptr(cm) if len(cm) else None, len(cm), opt(ci), opt(ki), opt(ys), opt(pf), count)
    return ctx, head, l, None if rp is None or count == 0 else _lib.ptr(rp), opt(gi), n_groups, (cm, ci, ki, ys, pf, rp, gi)


def coset_group_sums(commitments, commitment_indices, coset_indices, ys, proofs, n: int, srs, r_powers=None, ctx=None, groups="commitment",
                     n_groups=None):
    """The two G1 sums (L_g, R_g) of every group's own pairing equation (`kzg_coset_group_sums`): group g of the items is good iff
    e(L_g, [tau^l]_2) = e(R_g, G2), and the sums over all groups are the pair `verify_multiproof_batch` checks.  `groups` as for
    `locate_bad_multiproofs`.  Returns (lhs, lhs_is_infinity, rhs, rhs_is_infinity): (n_groups, 8) uint64 affine wire points and
    (n_groups,) bool arrays; an empty group gives the identity twice."""
    ctx, head, l, rp, gi, n_groups, _keep = _locate_args(commitments, commitment_indices, coset_indices, ys, proofs, srs, None, r_powers, ctx, groups,
                                                         n_groups, False)
    lhs, rhs = np.zeros((n_groups, 8), np.uint64), np.zeros((n_groups, 8), np.uint64)
    linf, rinf = np.zeros(max(n_groups, 1), np.uint8), np.zeros(max(n_groups, 1), np.uint8)
    rc = _lib.load().kzg_coset_group_sums(*head, int(n), l, rp, gi, n_groups, _lib.ptr(lhs) if n_groups else None, linf.ctypes.data_as(_lib.u8p),
                                          _lib.ptr(rhs) if n_groups else None, rinf.ctypes.data_as(_lib.u8p))
    _raise_for(rc, ctx)
    return lhs, linf[:n_groups].astype(bool), rhs, rinf[:n_groups].astype(bool)


def locate_bad_multiproofs(commitments, commitment_indices, coset_indices, ys, proofs, n: int, srs, g2_tau_l=None, r_powers=None, ctx=None,
                           groups="commitment", n_groups=None):
    """Which groups of a batch of coset proofs are bad (`kzg_verify_multiproof_batch_locate`): the group sums once on the GPU, then a
    search of the tree of those sums on the host, one pairing check per step and at most 1 + 2 b ceil(log2 n_groups) of them for b bad
    groups.  `groups` = "commitment" (group = commitment row, n_groups = number of commitments), "item" (one group per item) or an
    integer array of group indices with `n_groups`.  Returns (good, pairing_checks): a bool array of length n_groups (True = good) and
    the number of pairing checks; all True is the accept of `verify_multiproof_batch`.  This call always pays for the group sums: a
    caller who expects good batches calls `verify_multiproof_batch` first and this only after a reject."""
    ctx, head, l, rp, gi, n_groups, _keep = _locate_args(commitments, commitment_indices, coset_indices, ys, proofs, srs, g2_tau_l, r_powers, ctx, groups,
                                                         n_groups, True)
    good = np.zeros(max(n_groups, 1), np.uint8)
    bad, checks = _lib.sz(0), _lib.sz(0)
    rc = _lib.load().kzg_verify_multiproof_batch_locate(*head, int(n), l, rp, _g2_arg(g2_tau_l), gi, n_groups, good.ctypes.data_as(_lib.u8p), C.byref(bad),
                                                        C.byref(checks))
    _raise_for(rc, ctx)
    good = good[:n_groups].astype(bool)
    assert int(bad.value) == int((~good).sum())
    return good, int(checks.value)
