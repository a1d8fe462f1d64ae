"""Mirror of prover/src/kzg.rs `KZG`: same method names, argument meaning and error behaviour; the
G1 MSM and the Fr NTT/IFFT behind them run as HIP kernels through the C-ABI."""
import ctypes as C

import numpy as np

from . import _lib, helpers
from .errors import CommitError, FFTError, GenericError, InvalidInputLength, NotOnCurveError, SerializationError, SrsCapacityExceeded
from .fr import g1_is_identity
from .polynomial import PolynomialCoeffForm, PolynomialEvalForm


def _drain_slot(ctx, slot, proof=False):
    """Wait for an asynchronous call left in flight on `slot` and drop its result (generator clean-up paths)."""
    lib = _lib.load()
    out = np.zeros(8, dtype=np.uint64); inf = C.c_uint8(0); y = np.zeros(4, dtype=np.uint64)
    if proof:
        lib.kzg_compute_proof_end(ctx.handle, slot, _lib.ptr(out), C.byref(inf), _lib.ptr(y))
    else:
        lib.kzg_msm_g1_srs_end(ctx.handle, slot, _lib.ptr(out), C.byref(inf), None)


class KZG:
    def __init__(self, ctx=None):
        self.ctx = ctx
        self.expanded_roots_of_unity = np.zeros((0, 4), dtype=np.uint64)

    @classmethod
    def new(cls, ctx=None):
        return cls(ctx)

    def _ctx(self):
        if self.ctx is None:
            self.ctx = _lib.default_context()
        return self.ctx

    # kzg.rs:65-72
    def calculate_and_store_roots_of_unity(self, length_of_data_after_padding: int):
        self.expanded_roots_of_unity = helpers.calculate_roots_of_unity(length_of_data_after_padding, self._ctx())

    def get_roots_of_unities(self):
        return self.expanded_roots_of_unity.copy()

    def get_nth_root_of_unity(self, i):
        return self.expanded_roots_of_unity[i] if 0 <= i < len(self.expanded_roots_of_unity) else None

    # kzg.rs:84-104
    def commit_eval_form(self, polynomial: PolynomialEvalForm, srs):
        if len(polynomial) > len(srs):
            raise SrsCapacityExceeded(len(polynomial), len(srs))
        ctx = self._ctx()
        evals = _lib.as_u64(polynomial.evaluations(), 4)
        out = np.zeros(8, dtype=np.uint64); inf = C.c_uint8(0)
        rc = _lib.load().kzg_commit_eval_form(ctx.handle, srs.handle, _lib.ptr(evals), len(evals), _lib.ptr(out), C.byref(inf))
        if rc == _lib.ERR_NOT_POWER_OF_TWO:
            raise FFTError("length provided is not a power of 2")
        if rc == _lib.ERR_DOMAIN:
            raise FFTError("Could not perform IFFT due to domain consturction error")
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return out

    # kzg.rs:107-125
    def commit_coeff_form(self, polynomial: PolynomialCoeffForm, srs):
        if len(polynomial) > len(srs):
            raise SerializationError("polynomial length is not correct")
        ctx = self._ctx()
        coeffs = _lib.as_u64(polynomial.coeffs(), 4)
        out = np.zeros(8, dtype=np.uint64); inf = C.c_uint8(0)
        rc = _lib.load().kzg_commit_coeff_form(ctx.handle, srs.handle, _lib.ptr(coeffs), len(coeffs), _lib.ptr(out), C.byref(inf))
        if rc == _lib.ERR_MSM_LENGTH_MISMATCH:
            raise CommitError(str(min(len(coeffs), len(srs))))
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return out

    # ---- G2: the length commitment and the length proof of the protocol's blob header (G2SRS; csrc/g2msm.hip) ------------------
    def commit_g2_coeff_form(self, polynomial: PolynomialCoeffForm, g2_srs):
        """sum f_i [tau^i]_2 (`kzg_commit_g2_coeff_form`): a (16,) wire G2 point."""
        if len(polynomial) > len(g2_srs):
            raise SerializationError("polynomial length is not correct")
        ctx = self._ctx()
        coeffs = _lib.as_u64(polynomial.coeffs(), 4)
        out = np.zeros(16, dtype=np.uint64); inf = C.c_uint8(0)
        rc = _lib.load().kzg_commit_g2_coeff_form(ctx.handle, g2_srs.handle, _lib.ptr(coeffs), len(coeffs), _lib.ptr(out), C.byref(inf))
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return out

    def commit_g2_eval_form(self, polynomial: PolynomialEvalForm, g2_srs):
        """The same from evaluations: inverse NTT on the device, then the G2 MSM (`kzg_commit_g2_eval_form`)."""
        if len(polynomial) > len(g2_srs):
            raise SrsCapacityExceeded(len(polynomial), len(g2_srs))
        ctx = self._ctx()
        evals = _lib.as_u64(polynomial.evaluations(), 4)
        out = np.zeros(16, dtype=np.uint64); inf = C.c_uint8(0)
        rc = _lib.load().kzg_commit_g2_eval_form(ctx.handle, g2_srs.handle, _lib.ptr(evals), len(evals), _lib.ptr(out), C.byref(inf))
        if rc == _lib.ERR_NOT_POWER_OF_TWO:
            raise FFTError("length provided is not a power of 2")
        if rc == _lib.ERR_DOMAIN:
            raise FFTError("Could not perform IFFT due to domain consturction error")
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return out

    def commit_with_length_proof(self, polynomial: PolynomialCoeffForm, srs, g2_srs, g2_trailing, srs_order: int, claimed_len: int):
        """The blob header (`kzg_commit_with_length_proof`): (commitment (8,), length commitment (16,), length proof (16,)) of the
        coefficients for the claimed length d = claimed_len over a setup of order srs_order; g2_trailing holds
        [tau^(g2_trailing.first_power + i)]_2 and must cover the powers srs_order - d .. srs_order - 1.  One scalar upload, the G1
        commitment, and both G2 MSMs over one sort."""
        ctx = self._ctx()
        coeffs = _lib.as_u64(polynomial.coeffs(), 4)
        c = np.zeros(8, dtype=np.uint64); c2 = np.zeros(16, dtype=np.uint64); pi2 = np.zeros(16, dtype=np.uint64)
        rc = _lib.load().kzg_commit_with_length_proof(ctx.handle, srs.handle, g2_srs.handle, g2_trailing.handle, g2_trailing.first_power, srs_order,
                                                      _lib.ptr(coeffs), len(coeffs), claimed_len, _lib.ptr(c), _lib.ptr(c2), _lib.ptr(pi2))
        if rc == _lib.ERR_NOT_POWER_OF_TWO:
            raise FFTError("length provided is not a power of 2")
        if rc == _lib.ERR_SRS_CAPACITY_EXCEEDED:
            raise SrsCapacityExceeded(int(claimed_len), len(g2_trailing))
        if rc == _lib.ERR_POLY_LENGTH:
            raise SerializationError("polynomial length is not correct")
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return c, c2, pi2

    def commit_with_length_proof_batch(self, polys, srs, g2_srs, g2_trailing, srs_order: int, claimed_len: int):
        """The headers of B blobs of one length and one claimed length in ONE call (`kzg_commit_with_length_proof_batch`): arrays (B, 8),
        (B, 16), (B, 16) whose row b is `commit_with_length_proof` of polys[b], bit for bit.  One scalar upload; the G1 commitments are
        the batched commitments'; the G2 elements of a group of blobs come from one sort and one launch sequence (both base sets in every
        launch; `helpers.g2_batch_info` tells how a shape is grouped, `Context.set_g2_batch_group` caps the groups)."""
        ctx = self._ctx()
        rows = [_lib.as_u64(p.coeffs() if hasattr(p, "coeffs") else p, 4).reshape(-1, 4) for p in polys]
        count = len(rows)
        n = len(rows[0]) if rows else 0
        if any(len(r) != n for r in rows):
            raise GenericError("batched headers need polynomials of one length")
        data = np.ascontiguousarray(np.concatenate(rows, axis=0)) if n and count else np.zeros((0, 4), dtype=np.uint64)
        c = np.zeros((count, 8), dtype=np.uint64); c2 = np.zeros((count, 16), dtype=np.uint64); pi2 = np.zeros((count, 16), dtype=np.uint64)
        rc = _lib.load().kzg_commit_with_length_proof_batch(ctx.handle, srs.handle, g2_srs.handle, g2_trailing.handle, g2_trailing.first_power, srs_order,
                                                            _lib.ptr(data) if data.size else None, n, count, claimed_len, _lib.ptr(c), _lib.ptr(c2),
                                                            _lib.ptr(pi2))
        if rc == _lib.ERR_NOT_POWER_OF_TWO:
            raise FFTError("length provided is not a power of 2")
        if rc == _lib.ERR_SRS_CAPACITY_EXCEEDED:
            raise SrsCapacityExceeded(int(claimed_len), len(g2_trailing))
        if rc == _lib.ERR_POLY_LENGTH:
            raise SerializationError("polynomial length is not correct")
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return c, c2, pi2

    def commit_with_length_proof_batch_be(self, polys, srs, g2_srs, g2_trailing, srs_order: int, claimed_len: int):
        """`commit_with_length_proof_batch` in the serialized form a disperser sends (`verifier.encode_header_items`): (commitments_be,
        length_commitments_be, length_proofs_be) bytes, 32 / 64 / 64 per header, what `verifier.verify_length_proof_batch_bytes` takes."""
        from . import verifier
        return verifier.encode_header_items(*self.commit_with_length_proof_batch(polys, srs, g2_srs, g2_trailing, srs_order, claimed_len))

    # ---- batched commitments: many polynomials of one length against one SRS in one kernel sequence (no counterpart in the
    # reference, which commits one polynomial per call; same values as that many calls) -----------------------------------------
    def _commit_batch(self, rows, srs, eval_form):
        ctx = self._ctx()
        rows = [_lib.as_u64(r, 4).reshape(-1, 4) for r in rows]
        if not rows:
            return np.zeros((0, 8), dtype=np.uint64)
        n = len(rows[0])
        if any(len(r) != n for r in rows):
            raise GenericError("batched commitments need polynomials of one length")
        if n > len(srs):
            if eval_form:
                raise SrsCapacityExceeded(n, len(srs))
            raise SerializationError("polynomial length is not correct")
        data = np.ascontiguousarray(np.concatenate(rows, axis=0)) if n else np.zeros((0, 4), dtype=np.uint64)
        out = np.zeros((len(rows), 8), dtype=np.uint64)
        fn = _lib.load().kzg_commit_eval_form_batch if eval_form else _lib.load().kzg_commit_coeff_form_batch
        rc = fn(ctx.handle, srs.handle, _lib.ptr(data) if n else None, n, len(rows), _lib.ptr(out), None)
        ctx.check_device(rc)
        if rc == _lib.ERR_NOT_POWER_OF_TWO:
            raise FFTError("length provided is not a power of 2")
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return out

    def commit_coeff_form_batch(self, polynomials, srs):
        """commit_coeff_form of every polynomial (all of one length) in ONE call: (count, 8) wire points."""
        return self._commit_batch([p.coeffs() for p in polynomials], srs, False)

    def commit_eval_form_batch(self, polynomials, srs):
        """commit_eval_form of every polynomial (all of one padded length) in ONE call; the Lagrange basis of that length stays cached with the SRS."""
        return self._commit_batch([p.evaluations() for p in polynomials], srs, True)

    def commit_blob_batch(self, blobs, srs):
        """commit_blob (kzg.rs:182-185) of every blob; blobs whose polynomials differ in length are grouped by length."""
        polys = [b.to_polynomial_eval_form() for b in blobs]
        out = np.zeros((len(polys), 8), dtype=np.uint64)
        by_len = {}
        for i, p in enumerate(polys):
            by_len.setdefault(len(p), []).append(i)
        for _, idx in sorted(by_len.items()):
            res = self.commit_eval_form_batch([polys[i] for i in idx], srs)
            for i, r in zip(idx, res):
                out[i] = r
        return out

    # ---- streams of commitments, two in flight (kzg_*_begin(slot) / kzg_msm_g1_srs_end(slot)) --------------------------
    def _pipelined(self, items, begin):
        """begin(item, slot) -> status, or None when the item needs no device work (yields the identity)."""
        ctx = self._ctx()
        lib = _lib.load()

        def end(slot):
            out = np.zeros(8, dtype=np.uint64); inf = C.c_uint8(0)
            rc = lib.kzg_msm_g1_srs_end(ctx.handle, slot, _lib.ptr(out), C.byref(inf), None)
            ctx.check_device(rc)
            if rc != _lib.OK:
                raise CommitError(_lib.status_message(rc))
            return out

        prev = None
        k = 0
        try:
            for item in items:
                slot = k & 1
                rc = begin(item, slot)
                if rc is None:
                    if prev is not None:
                        p, prev = prev, None
                        yield end(p)
                    yield np.zeros(8, dtype=np.uint64)
                    continue
                k += 1
                if rc == _lib.ERR_SRS_CAPACITY_EXCEEDED:
                    raise SrsCapacityExceeded(len(item), 0)
                if rc == _lib.ERR_NOT_POWER_OF_TWO:
                    raise FFTError("length provided is not a power of 2")
                ctx.check_device(rc)
                if rc != _lib.OK:
                    raise CommitError(_lib.status_message(rc))
                if prev is not None:
                    p, prev = prev, slot
                    yield end(p)
                else:
                    prev = slot
            if prev is not None:
                p, prev = prev, None
                yield end(p)
        finally:
            # an exception in begin() for item k+1, or a consumer that stops early, must not leave a slot in flight: a pending
            # slot can never be begun again and slot 0 blocks every synchronous call of the context
            if prev is not None:
                _drain_slot(ctx, prev)

    def commit_coeff_form_stream(self, polynomials, srs):
        """`commit_coeff_form` over a stream of polynomials: the H2D copy and the sort of polynomial k+1 run beside the bucket
        accumulation of polynomial k.  Yields the commitments in order."""
        ctx = self._ctx()
        lib = _lib.load()

        def begin(polynomial, slot):
            if len(polynomial) > len(srs):
                raise SerializationError("polynomial length is not correct")
            coeffs = _lib.as_u64(polynomial.coeffs(), 4)
            if len(coeffs) == 0:
                return None
            return lib.kzg_msm_g1_srs_begin(ctx.handle, srs.handle, 0, _lib.ptr(coeffs), len(coeffs), slot)
        return self._pipelined(polynomials, begin)

    def commit_eval_form_stream(self, polynomials, srs):
        """`commit_eval_form` over a stream of evaluation-form polynomials (H2D, IFFT and MSM of each on its slot's stream)."""
        ctx = self._ctx()
        lib = _lib.load()

        def begin(polynomial, slot):
            ev = _lib.as_u64(polynomial.evaluations(), 4)
            if len(ev) > len(srs):
                raise SrsCapacityExceeded(len(ev), len(srs))
            return lib.kzg_commit_eval_form_begin(ctx.handle, srs.handle, _lib.ptr(ev), len(ev), slot)
        return self._pipelined(polynomials, begin)

    def commit_blob_stream(self, blobs, srs):
        """`commit_blob` over a stream of blobs: bytes in, points out, nothing but the 32-byte-per-element blob crosses PCIe."""
        ctx = self._ctx()
        lib = _lib.load()

        def begin(blob, slot):
            data = np.frombuffer(blob.data(), dtype=np.uint8)
            n = 1
            while n < -(-len(data) // 32):
                n <<= 1
            if n > len(srs):
                raise SrsCapacityExceeded(n, len(srs))
            return lib.kzg_commit_blob_begin(ctx.handle, srs.handle, data.ctypes.data_as(_lib.u8p) if len(data) else None, len(data), slot)
        return self._pipelined(blobs, begin)

    def compute_proof_stream(self, items, srs, want_y=False):
        """`compute_proof` over a stream of (polynomial, z_fr) pairs, two in flight (`kzg_compute_proof_begin` / `_end`): upload,
        batch inversion and quotient of proof k+1 run beside the MSM of proof k.  Yields proofs (or (proof, y)) in order."""
        ctx = self._ctx()
        lib = _lib.load()

        def end(slot):
            out = np.zeros(8, dtype=np.uint64); inf = C.c_uint8(0); y = np.zeros(4, dtype=np.uint64)
            rc = lib.kzg_compute_proof_end(ctx.handle, slot, _lib.ptr(out), C.byref(inf), _lib.ptr(y))
            ctx.check_device(rc)
            if rc != _lib.OK:
                raise GenericError(_lib.status_message(rc))
            return (out, y) if want_y else out

        prev = None
        try:
            for k, (polynomial, z_fr) in enumerate(items):
                ev = _lib.as_u64(polynomial.evaluations(), 4)
                z = np.ascontiguousarray(_lib.as_u64(z_fr, 0).reshape(4))
                slot = k & 1
                rc = lib.kzg_compute_proof_begin(ctx.handle, srs.handle, _lib.ptr(ev), len(ev), None, len(ev), _lib.ptr(z), slot)
                if rc == _lib.ERR_SRS_CAPACITY_EXCEEDED:
                    raise SrsCapacityExceeded(len(ev), len(srs))
                ctx.check_device(rc)
                if rc != _lib.OK:
                    raise GenericError(_lib.status_message(rc))
                if prev is not None:
                    p, prev = prev, slot
                    yield end(p)
                else:
                    prev = slot
            if prev is not None:
                p, prev = prev, None
                yield end(p)
        finally:
            if prev is not None:
                _drain_slot(ctx, prev, proof=True)

    # kzg.rs:182-185
    def commit_blob(self, blob, srs):
        """Bytes in, point out: bytes -> Fr, IFFT and MSM all on the device (`kzg_commit_blob`)."""
        ctx = self._ctx()
        data = blob.data()
        n_elems = -(-len(data) // 32)
        n = 1
        while n < n_elems:
            n <<= 1
        if n > len(srs):
            raise SrsCapacityExceeded(n, len(srs))
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
        out = np.zeros(8, dtype=np.uint64); inf = C.c_uint8(0)
        rc = _lib.load().kzg_commit_blob(ctx.handle, srs.handle, buf.ctypes.data_as(_lib.u8p), len(data), _lib.ptr(out), C.byref(inf))
        if rc == _lib.ERR_SRS_CAPACITY_EXCEEDED:
            raise SrsCapacityExceeded(n, len(srs))
        if rc == _lib.ERR_TOO_LARGE:
            raise GenericError("Input size exceeds maximum polynomial size")
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return out

    # kzg.rs:128-178
    def _compute_proof_impl(self, polynomial, z_fr, srs, want_y=False):
        if len(polynomial) != len(self.expanded_roots_of_unity):
            raise GenericError("inconsistent length between blob and root of unities")
        if len(polynomial) > len(srs):
            raise SrsCapacityExceeded(len(polynomial), len(srs))
        ctx = self._ctx()
        evals = _lib.as_u64(polynomial.evaluations(), 4)
        roots = _lib.as_u64(self.expanded_roots_of_unity, 4)
        z = _lib.as_u64(z_fr, 0).reshape(4)
        out = np.zeros(8, dtype=np.uint64); inf = C.c_uint8(0); y = np.zeros(4, dtype=np.uint64)
        rc = _lib.load().kzg_compute_proof(ctx.handle, srs.handle, _lib.ptr(evals), len(evals), _lib.ptr(roots), len(roots),
                                           _lib.ptr(z), _lib.ptr(out), C.byref(inf), _lib.ptr(y))
        if rc == _lib.ERR_ROOTS_LENGTH:
            raise GenericError("inconsistent length between blob and root of unities")
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return (out, y) if want_y else out

    # kzg.rs:215-234
    def compute_proof(self, polynomial, z_fr, srs):
        if len(polynomial) != len(self.expanded_roots_of_unity):
            raise GenericError("inconsistent length between blob and root of unities")
        return self._compute_proof_impl(polynomial, z_fr, srs)

    # kzg.rs:187-207
    def compute_proof_with_known_z_fr_index(self, polynomial, index: int, srs):
        if index < 0 or index >= 1 << 64:
            raise GenericError("Index conversion to usize failed")
        z = self.get_nth_root_of_unity(index)
        if z is None:
            raise GenericError("Root of unity not found")
        return self.compute_proof(polynomial, z, srs)

    # kzg.rs:187-234, every point at once (FK20)
    def compute_multiproofs(self, polynomial, srs, chunk_len: int = 1):
        """The proofs of every coset of the n-point domain in one call (`kzg_compute_multiproofs`, Feist-Khovratovich "FK20").
        Chunk k < m = n / chunk_len is the coset {w^(k + j m) : j < chunk_len}: evaluation indices k, k + m, k + 2m, ...; its proof is
        [f / (X^chunk_len - w^(k chunk_len))](tau).  With chunk_len = 1, row k is `compute_proof_with_known_z_fr_index(polynomial, k)`.
        Returns an (m, 8) uint64 array of wire points (the identity as zeros, as `compute_proof` returns it)."""
        if isinstance(polynomial, PolynomialEvalForm):
            data, eval_form = polynomial.evaluations(), 1
        elif isinstance(polynomial, PolynomialCoeffForm):
            data, eval_form = polynomial.coeffs(), 0
        else:
            raise TypeError("compute_multiproofs takes a PolynomialEvalForm or a PolynomialCoeffForm")
        n = len(polynomial)
        chunk_len = int(chunk_len)
        if n < 2:
            raise GenericError("multi-proofs need a polynomial of at least 2 elements")
        if chunk_len <= 0 or (chunk_len & (chunk_len - 1)) != 0:
            raise GenericError("chunk length is not a power of 2")
        if chunk_len > n // 2:
            raise GenericError("chunk length exceeds half the polynomial length")
        if n > len(srs):
            raise SrsCapacityExceeded(n, len(srs))
        ctx = self._ctx()
        data = _lib.as_u64(data, 4)
        m = n // chunk_len
        out = np.zeros((m, 8), dtype=np.uint64)
        inf = np.zeros(m, dtype=np.uint8)
        rc = _lib.load().kzg_compute_multiproofs(ctx.handle, srs.handle, _lib.ptr(data), n, eval_form, chunk_len, _lib.ptr(out),
                                                 inf.ctypes.data_as(_lib.u8p))
        if rc == _lib.ERR_NOT_POWER_OF_TWO:
            raise FFTError("length provided is not a power of 2")
        if rc == _lib.ERR_DOMAIN:
            raise FFTError("Could not perform IFFT due to domain consturction error")
        if rc == _lib.ERR_SRS_CAPACITY_EXCEEDED:
            raise SrsCapacityExceeded(n, len(srs))
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return out

    def encode_cosets(self, polynomial, srs, n: int, chunk_len: int = 1, values: bool = True, proofs: bool = True):
        """The encoder (`kzg_encode_cosets`): a polynomial of d elements (a PolynomialCoeffForm, or a PolynomialEvalForm on the d-point
        domain), evaluated on the domain of n = r d points and cut into the m = n / chunk_len cosets of `compute_multiproofs`, each
        with its proof.  Returns (ys, proofs): ys an (m, chunk_len, 4) array whose row k is row k of `cosets` of the n evaluations,
        proofs an (m, 8) array of wire points (the identity as zeros); `values=False` / `proofs=False` leaves that one out (None).
        The quotients have degree < d - chunk_len: `srs` needs d points, not n, and the FK20 table is `srs.cache_multiproof(d,
        chunk_len)`.  With n = d the proofs are those of `compute_multiproofs`."""
        if isinstance(polynomial, PolynomialEvalForm):
            data, eval_form = polynomial.evaluations(), 1
        elif isinstance(polynomial, PolynomialCoeffForm):
            data, eval_form = polynomial.coeffs(), 0
        else:
            raise TypeError("encode_cosets takes a PolynomialEvalForm or a PolynomialCoeffForm")
        d = len(polynomial)
        n = int(n)
        chunk_len = int(chunk_len)
        if not values and not proofs:
            raise GenericError("encode_cosets needs values, proofs or both")
        if d <= 0 or (d & (d - 1)) != 0 or n <= 0 or (n & (n - 1)) != 0:
            raise FFTError("length provided is not a power of 2")
        if n > 1 << 24:
            raise FFTError("Could not perform IFFT due to domain consturction error")
        if d < 2:
            raise GenericError("encode_cosets needs a polynomial of at least 2 elements")
        if d > n:
            raise GenericError("the domain is shorter than the polynomial")
        if chunk_len <= 0 or (chunk_len & (chunk_len - 1)) != 0:
            raise GenericError("chunk length is not a power of 2")
        if chunk_len > d // 2:
            raise GenericError("chunk length exceeds half the polynomial length")
        if d > len(srs):
            raise SrsCapacityExceeded(d, len(srs))
        ctx = self._ctx()
        data = _lib.as_u64(data, 4)
        m = n // chunk_len
        ys = np.zeros((m, chunk_len, 4), dtype=np.uint64) if values else None
        out = np.zeros((m, 8), dtype=np.uint64) if proofs else None
        inf = np.zeros(m, dtype=np.uint8)
        rc = _lib.load().kzg_encode_cosets(ctx.handle, srs.handle, _lib.ptr(data), d, eval_form, n, chunk_len,
                                           _lib.ptr(ys) if values else None, _lib.ptr(out) if proofs else None, inf.ctypes.data_as(_lib.u8p))
        if rc == _lib.ERR_NOT_POWER_OF_TWO:
            raise FFTError("length provided is not a power of 2")
        if rc == _lib.ERR_DOMAIN:
            raise FFTError("Could not perform IFFT due to domain consturction error")
        if rc == _lib.ERR_SRS_CAPACITY_EXCEEDED:
            raise SrsCapacityExceeded(d, len(srs))
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return ys, out

    def encode_cosets_batch(self, polynomials, srs, n: int, chunk_len: int = 1, values: bool = True, proofs: bool = True, eval_form=None):
        """`encode_cosets` for B blobs of one shape in one call (`kzg_encode_cosets_batch`): `polynomials` is a list of
        PolynomialCoeffForm or of PolynomialEvalForm of one length d, or one (B, d, 4) array of wire elements with `eval_form=` True /
        False.  Returns (ys, proofs): ys (B, m, chunk_len, 4), proofs (B, m, 8), row b bit-identical to `encode_cosets` of blob b;
        `values=False` / `proofs=False` leaves that one out (None).  The library works through the blobs in groups whose device
        workspace fits `Context.set_encode_group_bytes` (`helpers.encode_batch_info` tells how a shape is grouped and planned)."""
        if isinstance(polynomials, np.ndarray):
            if eval_form is None:
                raise TypeError("encode_cosets_batch of an array needs eval_form=True or False")
            data = _lib.as_u64(polynomials, 4)
            if polynomials.ndim != 3 or polynomials.shape[2] != 4:
                raise GenericError("encode_cosets_batch takes a (B, d, 4) array")
            count, d = int(polynomials.shape[0]), int(polynomials.shape[1])
            ef = 1 if eval_form else 0
        else:
            polys = list(polynomials)
            if polys and all(isinstance(q, PolynomialEvalForm) for q in polys):
                ef, rows = 1, [q.evaluations() for q in polys]
            elif polys and all(isinstance(q, PolynomialCoeffForm) for q in polys):
                ef, rows = 0, [q.coeffs() for q in polys]
            elif not polys:
                raise GenericError("encode_cosets_batch needs at least one polynomial")
            else:
                raise TypeError("encode_cosets_batch takes polynomials of one form: PolynomialEvalForm or PolynomialCoeffForm")
            if eval_form is not None and bool(eval_form) != bool(ef):
                raise TypeError("eval_form= contradicts the polynomials' form")
            count, d = len(polys), len(polys[0])
            if any(len(q) != d for q in polys):
                raise GenericError("encode_cosets_batch needs polynomials of one length")
            data = np.ascontiguousarray(np.stack([_lib.as_u64(r, 4) for r in rows]), dtype=np.uint64) if d else np.zeros((count, 0, 4), dtype=np.uint64)
        n = int(n)
        chunk_len = int(chunk_len)
        if count <= 0:
            raise GenericError("encode_cosets_batch needs at least one polynomial")
        if not values and not proofs:
            raise GenericError("encode_cosets needs values, proofs or both")
        if d <= 0 or (d & (d - 1)) != 0 or n <= 0 or (n & (n - 1)) != 0:
            raise FFTError("length provided is not a power of 2")
        if n > 1 << 24:
            raise FFTError("Could not perform IFFT due to domain consturction error")
        if d < 2:
            raise GenericError("encode_cosets needs a polynomial of at least 2 elements")
        if d > n:
            raise GenericError("the domain is shorter than the polynomial")
        if chunk_len <= 0 or (chunk_len & (chunk_len - 1)) != 0:
            raise GenericError("chunk length is not a power of 2")
        if chunk_len > d // 2:
            raise GenericError("chunk length exceeds half the polynomial length")
        if d > len(srs):
            raise SrsCapacityExceeded(d, len(srs))
        ctx = self._ctx()
        m = n // chunk_len
        ys = np.zeros((count, m, chunk_len, 4), dtype=np.uint64) if values else None
        out = np.zeros((count, m, 8), dtype=np.uint64) if proofs else None
        inf = np.zeros(count * m, dtype=np.uint8)
        rc = _lib.load().kzg_encode_cosets_batch(ctx.handle, srs.handle, _lib.ptr(data), count, d, ef, n, chunk_len,
                                                 _lib.ptr(ys) if values else None, _lib.ptr(out) if proofs else None, inf.ctypes.data_as(_lib.u8p))
        if rc == _lib.ERR_NOT_POWER_OF_TWO:
            raise FFTError("length provided is not a power of 2")
        if rc == _lib.ERR_DOMAIN:
            raise FFTError("Could not perform IFFT due to domain consturction error")
        if rc == _lib.ERR_SRS_CAPACITY_EXCEEDED:
            raise SrsCapacityExceeded(d, len(srs))
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return ys, out

    def encode_cosets_be(self, polynomial, srs, n: int, chunk_len: int = 1):
        """`encode_cosets` in the serialized form a disperser sends (`verifier.encode_coset_items`): (ys_be, proofs_be) bytes, 32 per value
        (big-endian) and per proof (gnark-compressed), what `verifier.verify_multiproof_batch_bytes` takes."""
        from . import verifier
        ys, proofs = self.encode_cosets(polynomial, srs, n, chunk_len)
        return verifier.encode_coset_items(ys, proofs)

    @staticmethod
    def _blob_rows_be(name, blobs):
        """(uint8 buffer, B, d) of blobs of 32-byte big-endian field elements: one `bytes` / `Blob` (B = 1), a list of them of one
        length, or a (B, d * 32) uint8 array."""
        if isinstance(blobs, np.ndarray):
            if blobs.dtype != np.uint8 or blobs.ndim != 2:
                raise GenericError("%s takes a (B, d * 32) uint8 array" % name)
            buf, count = np.ascontiguousarray(blobs).reshape(-1), int(blobs.shape[0])
            row = int(blobs.shape[1])
        else:
            if isinstance(blobs, (bytes, bytearray, memoryview)) or hasattr(blobs, "data"):
                blobs = [blobs]
            rows = [bytes(b.data()) if hasattr(b, "data") else bytes(b) for b in blobs]
            count = len(rows)
            row = len(rows[0]) if rows else 0
            if any(len(r) != row for r in rows):
                raise GenericError("%s needs blobs of one length" % name)
            buf = np.frombuffer(b"".join(rows), dtype=np.uint8)
        if count <= 0:
            raise GenericError("%s needs at least one blob" % name)
        if row == 0 or row % 32 != 0:
            raise InvalidInputLength()
        return buf, count, row // 32

    @staticmethod
    def _encode_shape_checks(d, n, chunk_len, srs):
        if d <= 0 or (d & (d - 1)) != 0 or n <= 0 or (n & (n - 1)) != 0:
            raise FFTError("length provided is not a power of 2")
        if n > 1 << 24:
            raise FFTError("Could not perform IFFT due to domain consturction error")
        if d < 2:
            raise GenericError("encode_cosets needs a polynomial of at least 2 elements")
        if d > n:
            raise GenericError("the domain is shorter than the polynomial")
        if chunk_len <= 0 or (chunk_len & (chunk_len - 1)) != 0:
            raise GenericError("chunk length is not a power of 2")
        if chunk_len > d // 2:
            raise GenericError("chunk length exceeds half the polynomial length")
        if d > len(srs):
            raise SrsCapacityExceeded(d, len(srs))

    @staticmethod
    def _raise_encode_bytes_status(ctx, rc, bad, d, srs):
        if rc == _lib.ERR_DESERIALIZE:
            raise SerializationError("blob %d, element %d: not a canonical field element (an integer not below r)" % (bad // d, bad % d))
        if rc == _lib.ERR_NOT_POWER_OF_TWO:
            raise FFTError("length provided is not a power of 2")
        if rc == _lib.ERR_DOMAIN:
            raise FFTError("Could not perform IFFT due to domain consturction error")
        if rc == _lib.ERR_SRS_CAPACITY_EXCEEDED:
            raise SrsCapacityExceeded(d, len(srs))
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))

    def encode_cosets_batch_bytes(self, blobs, srs, n: int, chunk_len: int = 1, eval_form: bool = False, commitments: bool = True, values: bool = True,
                                  proofs: bool = True):
        """`encode_cosets_batch` from blobs to the bytes a disperser sends, the codec inside the call (`kzg_encode_cosets_batch_bytes`).
        `blobs`: `bytes`, `Blob` objects (a list of one length, or one) or a (B, d * 32) uint8 array of 32-byte big-endian field elements,
        coefficients or (eval_form=True) evaluations.  Returns (commitments_be, ys_be, proofs_be): B x 32, B x n x 32 and B x m x 32 bytes
        (None where the keyword is False): byte for byte `verifier.encode_coset_items` of `encode_cosets_batch` on the decoded blobs, and
        the compressed commitments of their coefficients.  An element not below r raises SerializationError naming the blob and the
        element; everything else as `encode_cosets_batch`."""
        buf, count, d = self._blob_rows_be("encode_cosets_batch_bytes", blobs)
        n, chunk_len = int(n), int(chunk_len)
        if not commitments and not values and not proofs:
            raise GenericError("encode_cosets needs commitments, values, proofs or any of them")
        self._encode_shape_checks(d, n, chunk_len, srs)
        ctx = self._ctx()
        m = n // chunk_len
        cm = np.zeros(count * 32, dtype=np.uint8) if commitments else None
        ys = np.zeros(count * n * 32, dtype=np.uint8) if values else None
        pr = np.zeros(count * m * 32, dtype=np.uint8) if proofs else None
        p8 = lambda a: a.ctypes.data_as(_lib.u8p) if a is not None else None
        bad = C.c_uint64(0)
        rc = _lib.load().kzg_encode_cosets_batch_bytes(ctx.handle, srs.handle, p8(buf), count, d, 1 if eval_form else 0, n, chunk_len, p8(cm), p8(ys), p8(pr),
                                                       C.byref(bad))
        self._raise_encode_bytes_status(ctx, rc, bad.value, d, srs)
        return tuple(a.tobytes() if a is not None else None for a in (cm, ys, pr))

    def disperse_blobs_bytes(self, blobs, srs, g2_srs, g2_trailing, srs_order: int, claimed_len: int, n: int, chunk_len: int = 1, values: bool = True,
                             proofs: bool = True):
        """The disperser's call (`kzg_disperse_blobs_bytes`): from blobs of 32-byte big-endian coefficients (as `encode_cosets_batch_bytes`
        takes them) to everything that leaves for the network.  Returns (commitments_be, length_commitments_be, length_proofs_be, ys_be,
        proofs_be): the three header arrays are byte for byte `commit_with_length_proof_batch_be` on the decoded blobs (32 / 64 / 64
        bytes per blob), the chunks those of `encode_cosets_batch_bytes` (None where the keyword is False).  One upload, as bytes; the
        decoded coefficients feed the encoder, the G1 commitments and the G2 MSMs.  Errors as `encode_cosets_batch_bytes` and
        `commit_with_length_proof_batch`."""
        buf, count, d = self._blob_rows_be("disperse_blobs_bytes", blobs)
        n, chunk_len = int(n), int(chunk_len)
        self._encode_shape_checks(d, n, chunk_len, srs)
        srs_order, claimed_len = int(srs_order), int(claimed_len)
        if srs_order <= 0 or (srs_order & (srs_order - 1)) != 0 or claimed_len <= 0 or (claimed_len & (claimed_len - 1)) != 0:
            raise FFTError("length provided is not a power of 2")
        if d > claimed_len or claimed_len > srs_order:
            raise GenericError("the claimed length must lie between the polynomial's length and the order of the setup")
        ctx = self._ctx()
        m = n // chunk_len
        cm = np.zeros(count * 32, dtype=np.uint8); c2 = np.zeros(count * 64, dtype=np.uint8); pi2 = np.zeros(count * 64, dtype=np.uint8)
        ys = np.zeros(count * n * 32, dtype=np.uint8) if values else None
        pr = np.zeros(count * m * 32, dtype=np.uint8) if proofs else None
        p8 = lambda a: a.ctypes.data_as(_lib.u8p) if a is not None else None
        bad = C.c_uint64(0)
        rc = _lib.load().kzg_disperse_blobs_bytes(ctx.handle, srs.handle, g2_srs.handle, g2_trailing.handle, g2_trailing.first_power, int(srs_order), p8(buf), count, d,
                                                  n, chunk_len, int(claimed_len), p8(cm), p8(c2), p8(pi2), p8(ys), p8(pr), C.byref(bad))
        if rc == _lib.ERR_SRS_CAPACITY_EXCEEDED:
            raise SrsCapacityExceeded(int(claimed_len), len(g2_trailing))
        if rc == _lib.ERR_POLY_LENGTH:
            raise SerializationError("polynomial length is not correct")
        self._raise_encode_bytes_status(ctx, rc, bad.value, d, srs)
        return tuple(a.tobytes() if a is not None else None for a in (cm, c2, pi2, ys, pr))

    @staticmethod
    def _coset_items_polys(name, polynomials, eval_form):
        """(data (B, d, 4), count, d, eval_form flag) of the polynomials of `prove_cosets_batch` / `coset_quotients`: one polynomial, a list
        of one form and length, or a (B, d, 4) array with eval_form= True / False."""
        if isinstance(polynomials, (PolynomialEvalForm, PolynomialCoeffForm)):
            polynomials = [polynomials]
        if isinstance(polynomials, np.ndarray):
            if eval_form is None:
                raise TypeError("%s of an array needs eval_form=True or False" % name)
            if polynomials.ndim != 3 or polynomials.shape[2] != 4:
                raise GenericError("%s takes a (B, d, 4) array" % name)
            return np.ascontiguousarray(polynomials, dtype=np.uint64), int(polynomials.shape[0]), int(polynomials.shape[1]), 1 if eval_form else 0
        polys = list(polynomials)
        if polys and all(isinstance(q, PolynomialEvalForm) for q in polys):
            ef, rows = 1, [q.evaluations() for q in polys]
        elif polys and all(isinstance(q, PolynomialCoeffForm) for q in polys):
            ef, rows = 0, [q.coeffs() for q in polys]
        elif not polys:
            raise GenericError("%s needs at least one polynomial" % name)
        else:
            raise TypeError("%s takes polynomials of one form: PolynomialEvalForm or PolynomialCoeffForm" % name)
        if eval_form is not None and bool(eval_form) != bool(ef):
            raise TypeError("eval_form= contradicts the polynomials' form")
        d = len(polys[0])
        if any(len(q) != d for q in polys):
            raise GenericError("%s needs polynomials of one length" % name)
        data = np.ascontiguousarray(np.stack([_lib.as_u64(r, 4) for r in rows]), dtype=np.uint64) if d else np.zeros((len(polys), 0, 4), dtype=np.uint64)
        return data, len(polys), d, ef

    @staticmethod
    def _coset_items_check(count, d, n, chunk_len, poly_indices, coset_indices, srs_len):
        """The argument errors of `encode_cosets`, then the items: (poly index array or None, coset index array)."""
        if d <= 0 or (d & (d - 1)) != 0 or n <= 0 or (n & (n - 1)) != 0:
            raise FFTError("length provided is not a power of 2")
        if n > 1 << 24:
            raise FFTError("Could not perform IFFT due to domain consturction error")
        if d < 2:
            raise GenericError("encode_cosets needs a polynomial of at least 2 elements")
        if d > n:
            raise GenericError("the domain is shorter than the polynomial")
        if chunk_len <= 0 or (chunk_len & (chunk_len - 1)) != 0:
            raise GenericError("chunk length is not a power of 2")
        if chunk_len > d // 2:
            raise GenericError("chunk length exceeds half the polynomial length")
        if srs_len is not None and d > srs_len:
            raise SrsCapacityExceeded(d, srs_len)
        ks = np.ascontiguousarray(np.asarray(coset_indices, dtype=np.int64).reshape(-1))
        ps = None if poly_indices is None else np.ascontiguousarray(np.asarray(poly_indices, dtype=np.int64).reshape(-1))
        if ps is not None and len(ps) != len(ks):
            raise GenericError("one polynomial index per coset index")
        m = n // chunk_len
        if len(ks) and (int(ks.min()) < 0 or int(ks.max()) >= m):
            raise GenericError("coset indices must be below n / chunk length")
        if ps is not None and len(ps) and (int(ps.min()) < 0 or int(ps.max()) >= count):
            raise GenericError("polynomial indices must be below the number of polynomials")
        return (None if ps is None else ps.astype(np.uint64)), ks.astype(np.uint64)

    @staticmethod
    def _coset_items_status(ctx, rc, d, srs_len):
        """The status of `kzg_prove_cosets` / `kzg_coset_quotients` as `encode_cosets` raises it (KZG_ERR_INVALID_ARG: ValueError)."""
        if rc == _lib.ERR_NOT_POWER_OF_TWO:
            raise FFTError("length provided is not a power of 2")
        if rc == _lib.ERR_DOMAIN:
            raise FFTError("Could not perform IFFT due to domain consturction error")
        if rc == _lib.ERR_SRS_CAPACITY_EXCEEDED:
            raise SrsCapacityExceeded(d, srs_len)
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))

    def prove_cosets_batch(self, polynomials, srs, n: int, poly_indices, coset_indices, chunk_len: int = 1, values: bool = True,
                           proofs: bool = True, eval_form=None):
        """The values and proofs of selected cosets (`kzg_prove_cosets`), without the FK20 pipeline that computes every proof: item i is
        coset `coset_indices[i]` of `polynomials[poly_indices[i]]` (`poly_indices=None`: of polynomial 0).  `polynomials` is as in
        `encode_cosets_batch`.  Returns (ys, proofs): ys (n_items, chunk_len, 4), proofs (n_items, 8), row i bit-identical to row
        `coset_indices[i]` of `encode_cosets` on that polynomial; `values=False` / `proofs=False` leaves that one out (None).  Duplicate
        items are allowed.  The library works through the items in groups whose device workspace fits `Context.set_encode_group_bytes`
        (`helpers.prove_cosets_info` tells the grouping and the passes)."""
        data, count, d, ef = self._coset_items_polys("prove_cosets_batch", polynomials, eval_form)
        n = int(n)
        chunk_len = int(chunk_len)
        if not values and not proofs:
            raise GenericError("prove_cosets needs values, proofs or both")
        ps, ks = self._coset_items_check(count, d, n, chunk_len, poly_indices, coset_indices, len(srs))
        k = len(ks)
        ctx = self._ctx()
        ys = np.zeros((k, chunk_len, 4), dtype=np.uint64) if values else None
        out = np.zeros((k, 8), dtype=np.uint64) if proofs else None
        inf = np.zeros(max(k, 1), dtype=np.uint8)
        bad = C.c_uint64(0)
        rc = _lib.load().kzg_prove_cosets(ctx.handle, srs.handle, _lib.ptr(data), count, d, ef, n, chunk_len, None if ps is None else _lib.ptr(ps),
                                          _lib.ptr(ks), k, _lib.ptr(ys) if values else None, _lib.ptr(out) if proofs else None,
                                          inf.ctypes.data_as(_lib.u8p), C.byref(bad))
        self._coset_items_status(ctx, rc, d, len(srs))
        return ys, out

    def prove_cosets(self, polynomial, srs, n: int, coset_indices, chunk_len: int = 1, values: bool = True, proofs: bool = True):
        """`prove_cosets_batch` on one polynomial (a PolynomialCoeffForm, or a PolynomialEvalForm on the d-point domain): the rows
        `coset_indices` of `encode_cosets(polynomial, srs, n, chunk_len)`, in that order, at the cost of one division and one commitment
        per coset."""
        if not isinstance(polynomial, (PolynomialEvalForm, PolynomialCoeffForm)):
            raise TypeError("prove_cosets takes a PolynomialEvalForm or a PolynomialCoeffForm")
        return self.prove_cosets_batch([polynomial], srs, n, None, coset_indices, chunk_len, values, proofs)

    def coset_quotients(self, polynomials, n: int, poly_indices, coset_indices, chunk_len: int = 1, quotients: bool = True, values: bool = False,
                        eval_form=None):
        """The quotient polynomials behind `prove_cosets_batch` (`kzg_coset_quotients`; no SRS): returns (q, ys) with q an (n_items, d, 4)
        array, row i the coefficients of f / (X^chunk_len - w^(k chunk_len)) for item i (the top chunk_len of them zero), and ys the
        values as in `prove_cosets_batch`; `quotients=False` / `values=False` leaves that one out (None)."""
        data, count, d, ef = self._coset_items_polys("coset_quotients", polynomials, eval_form)
        n = int(n)
        chunk_len = int(chunk_len)
        if not quotients and not values:
            raise GenericError("coset_quotients needs quotients, values or both")
        ps, ks = self._coset_items_check(count, d, n, chunk_len, poly_indices, coset_indices, None)
        k = len(ks)
        ctx = self._ctx()
        q = np.zeros((k, d, 4), dtype=np.uint64) if quotients else None
        ys = np.zeros((k, chunk_len, 4), dtype=np.uint64) if values else None
        bad = C.c_uint64(0)
        rc = _lib.load().kzg_coset_quotients(ctx.handle, _lib.ptr(data), count, d, ef, n, chunk_len, None if ps is None else _lib.ptr(ps), _lib.ptr(ks), k,
                                             _lib.ptr(q) if quotients else None, _lib.ptr(ys) if values else None, C.byref(bad))
        self._coset_items_status(ctx, rc, d, 0)
        return q, ys

    def cosets(self, polynomial_eval_form, chunk_len: int = 1) -> np.ndarray:
        """The values that go with the proofs of `compute_multiproofs`: an (m, chunk_len, 4) array, m = n / chunk_len, whose row k is
        evals[k::m], the evaluations on the coset {w^(k + j m) : j < chunk_len} -- what `verifier.verify_multiproof*` takes as `ys`."""
        if not isinstance(polynomial_eval_form, PolynomialEvalForm):
            raise TypeError("cosets takes a PolynomialEvalForm")
        n = len(polynomial_eval_form)
        chunk_len = int(chunk_len)
        if chunk_len <= 0 or (chunk_len & (chunk_len - 1)) != 0:
            raise GenericError("chunk length is not a power of 2")
        if n < 2 or (n & (n - 1)) != 0 or chunk_len > n // 2:
            raise GenericError("chunk length exceeds half the polynomial length")
        ev = _lib.as_u64(polynomial_eval_form.evaluations(), 4).reshape(chunk_len, n // chunk_len, 4)     # [j][k] = evals[k + j m]
        return np.ascontiguousarray(ev.transpose(1, 0, 2))

    def recover_from_cosets(self, coset_indices, ys, n: int, degree_bound=None, eval_form: bool = True):
        """Erasure decoding (`kzg_recover_from_cosets`): the polynomial of degree < count * chunk_len through the values of `count`
        distinct cosets of the n-point domain.  `ys` is a (count, chunk_len, 4) array whose row i holds the values of coset
        `coset_indices[i]` (row `coset_indices[i]` of `cosets`), in any order.  Returns a PolynomialEvalForm of n evaluations, or with
        eval_form=False a PolynomialCoeffForm of n coefficients.  `degree_bound` (None or 0: count * chunk_len) is the degree bound the
        polynomial is known to have: values that are not those of a polynomial below it raise GenericError."""
        ys = np.ascontiguousarray(ys, dtype=np.uint64)
        idx = np.ascontiguousarray(coset_indices, dtype=np.uint64).reshape(-1)
        n = int(n)
        if ys.ndim != 3 or ys.shape[2] != 4 or ys.shape[0] != len(idx):
            raise GenericError("ys must have the shape (count, chunk_len, 4) with one row per coset index")
        count, chunk_len = int(ys.shape[0]), int(ys.shape[1])
        if n < 2 or (n & (n - 1)) != 0:
            raise FFTError("length provided is not a power of 2")
        if chunk_len <= 0 or (chunk_len & (chunk_len - 1)) != 0:
            raise GenericError("chunk length is not a power of 2")
        if chunk_len > n // 2:
            raise GenericError("chunk length exceeds half the polynomial length")
        m = n // chunk_len
        if count == 0 or count > m:
            raise GenericError("the number of cosets must be between 1 and n / chunk length")
        seen = np.zeros(m, dtype=bool)
        if int(idx.max()) < m:
            seen[idx.astype(np.int64)] = True
        if int(seen.sum()) != count:                                                          # an index >= m, or the same coset twice
            raise GenericError("coset indices must be distinct and below n / chunk length")
        bound = count * chunk_len if not degree_bound else int(degree_bound)               # None or 0: the default, as in the C-ABI
        if bound < 0 or bound > count * chunk_len:
            raise GenericError("too few cosets for the degree bound")
        ctx = self._ctx()
        out = np.zeros((n, 4), dtype=np.uint64)
        consistent = C.c_int32(0)
        rc = _lib.load().kzg_recover_from_cosets(ctx.handle, _lib.ptr(ys), _lib.ptr(idx), count, n, chunk_len, bound, 1 if eval_form else 0,
                                                 _lib.ptr(out), C.byref(consistent))
        if rc == _lib.ERR_DOMAIN:
            raise FFTError("Could not perform IFFT due to domain consturction error")
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        if not consistent.value:
            raise GenericError("the cosets are not the values of a polynomial below the degree bound")
        return PolynomialEvalForm(out) if eval_form else PolynomialCoeffForm(out)

    def recover_from_cosets_batch(self, coset_indices, ys, n: int, degree_bound=None, eval_form: bool = True, out_len=None):
        """`recover_from_cosets` for B blobs of one shape in one call (`kzg_recover_from_cosets_batch`).  `ys` is a (B, count, chunk_len, 4)
        array; `coset_indices` has the shape (count,), the cosets every blob has, or (B, count), row b those of blob b.  Returns
        (array (B, out_len, 4), consistent): row b is bit-identical to `recover_from_cosets` of blob b, evaluations or with
        eval_form=False coefficients, and `consistent` is a bool array (B,).  Unlike the single call this one does NOT raise on values that
        are not those of a polynomial below `degree_bound`: consistent[b] is False and row b is still the interpolant.  `out_len` (None
        or 0: n; coefficients only) keeps the first out_len >= degree bound coefficients of each blob.  The library works through the
        blobs in groups whose device workspace fits `Context.set_recover_group_bytes` (`helpers.recover_batch_info`)."""
        ys = np.ascontiguousarray(ys, dtype=np.uint64)
        idx = np.ascontiguousarray(coset_indices, dtype=np.uint64)
        n = int(n)
        if ys.ndim != 4 or ys.shape[3] != 4 or ys.shape[0] == 0:
            raise GenericError("ys must have the shape (B, count, chunk_len, 4) with B >= 1")
        blobs, count, chunk_len = int(ys.shape[0]), int(ys.shape[1]), int(ys.shape[2])
        if idx.shape not in ((count,), (blobs, count)):
            raise GenericError("coset indices must have the shape (count,) or (B, count)")
        index_rows = 1 if idx.ndim == 1 else blobs
        if n < 2 or (n & (n - 1)) != 0:
            raise FFTError("length provided is not a power of 2")
        if chunk_len <= 0 or (chunk_len & (chunk_len - 1)) != 0:
            raise GenericError("chunk length is not a power of 2")
        if chunk_len > n // 2:
            raise GenericError("chunk length exceeds half the polynomial length")
        m = n // chunk_len
        if count == 0 or count > m:
            raise GenericError("the number of cosets must be between 1 and n / chunk length")
        bound = count * chunk_len if not degree_bound else int(degree_bound)               # None or 0: the default, as in the C-ABI
        if bound < 0 or bound > count * chunk_len:
            raise GenericError("too few cosets for the degree bound")
        rows = n if not out_len else int(out_len)
        if rows != n and (eval_form or not bound <= rows <= n):
            raise GenericError("out_len is for coefficients, between the degree bound and n")
        ctx = self._ctx()
        out = np.zeros((blobs, rows, 4), dtype=np.uint64)
        consistent = np.zeros(blobs, dtype=np.int32)
        rc = _lib.load().kzg_recover_from_cosets_batch(ctx.handle, _lib.ptr(ys), _lib.ptr(idx), index_rows, blobs, count, n, chunk_len, bound,
                                                       1 if eval_form else 0, rows, _lib.ptr(out), consistent.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc == _lib.ERR_DOMAIN:
            raise FFTError("Could not perform IFFT due to domain consturction error")
        if rc == _lib.ERR_INVALID_ARG:                                                        # an index >= m, or the same coset twice in a row
            raise GenericError("coset indices must be distinct and below n / chunk length")
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return out, consistent.astype(bool)

    def recover_from_cosets_batch_bytes(self, coset_indices, ys_be, n: int, chunk_len: int, degree_bound=None, eval_form: bool = True, out_len=None):
        """`recover_from_cosets_batch` on chunks as they come off the wire, the codec inside the call
        (`kzg_recover_from_cosets_batch_bytes`): `ys_be` holds B x count x chunk_len big-endian values of 32 bytes, `coset_indices` has the
        shape (count,) or (B, count).  Returns (bytes, consistent): B x out_len x 32 bytes, row b byte for byte `encode_coset_items` of row
        b of `recover_from_cosets_batch` on the decoded values, and a bool array (B,).  A value not below r raises DeserializationError
        naming its item b * count + i.  Everything else as `recover_from_cosets_batch`."""
        idx = np.ascontiguousarray(coset_indices, dtype=np.uint64)
        n, chunk_len = int(n), int(chunk_len)
        if idx.ndim not in (1, 2) or idx.shape[-1] == 0:
            raise GenericError("coset indices must have the shape (count,) or (B, count)")
        count = int(idx.shape[-1])
        if n < 2 or (n & (n - 1)) != 0:
            raise FFTError("length provided is not a power of 2")
        if chunk_len <= 0 or (chunk_len & (chunk_len - 1)) != 0:
            raise GenericError("chunk length is not a power of 2")
        if chunk_len > n // 2:
            raise GenericError("chunk length exceeds half the polynomial length")
        buf = np.frombuffer(bytes(ys_be), dtype=np.uint8) if not isinstance(ys_be, np.ndarray) else np.ascontiguousarray(ys_be, dtype=np.uint8).reshape(-1)
        per_blob = count * chunk_len * 32
        if len(buf) == 0 or len(buf) % per_blob != 0:
            raise InvalidInputLength()
        blobs = len(buf) // per_blob
        if idx.ndim == 2 and idx.shape[0] != blobs:
            raise GenericError("coset indices must have the shape (count,) or (B, count)")
        index_rows = 1 if idx.ndim == 1 else blobs
        if count > n // chunk_len:
            raise GenericError("the number of cosets must be between 1 and n / chunk length")
        bound = count * chunk_len if not degree_bound else int(degree_bound)               # None or 0: the default, as in the C-ABI
        if bound < 0 or bound > count * chunk_len:
            raise GenericError("too few cosets for the degree bound")
        rows = n if not out_len else int(out_len)
        if rows != n and (eval_form or not bound <= rows <= n):
            raise GenericError("out_len is for coefficients, between the degree bound and n")
        ctx = self._ctx()
        out = np.zeros(blobs * rows * 32, dtype=np.uint8)
        consistent = np.zeros(blobs, dtype=np.int32)
        bad = C.c_uint64(0)
        rc = _lib.load().kzg_recover_from_cosets_batch_bytes(ctx.handle, buf.ctypes.data_as(_lib.u8p), _lib.ptr(idx), index_rows, blobs, count, n, chunk_len, bound,
                                                             1 if eval_form else 0, rows, out.ctypes.data_as(_lib.u8p),
                                                             consistent.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(bad))
        if rc == _lib.ERR_DESERIALIZE:
            helpers.raise_for_decode(rc, "value of item", bad.value, ctx)
        if rc == _lib.ERR_DOMAIN:
            raise FFTError("Could not perform IFFT due to domain consturction error")
        if rc == _lib.ERR_INVALID_ARG:                                                        # an index >= m, the same coset twice in a row, or slot 0 busy
            raise GenericError("coset indices must be distinct and below n / chunk length (or slot 0 is in flight)")
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return out.tobytes(), consistent.astype(bool)

    # kzg.rs:237-260
    def compute_quotient_eval_on_domain(self, z_fr, eval_fr, value_fr):
        """sum over the stored roots w^i != z of (f_i - value) w^i / ((z - w^i) z): the quotient's evaluation at the domain point z, on the GPU
        (`kzg_compute_quotient_eval_on_domain`).  Like the reference it reads one evaluation per stored root."""
        n = len(self.expanded_roots_of_unity)
        ev = _lib.as_u64(eval_fr, 4).reshape(-1, 4)
        if len(ev) < n:
            raise IndexError("index out of bounds: the len is %d but the index is %d" % (len(ev), len(ev)))      # eval_fr[i] in the reference's loop
        if n == 0:
            return np.zeros(4, dtype=np.uint64)
        ctx = self._ctx()
        out = np.zeros(4, dtype=np.uint64)
        ev = np.ascontiguousarray(ev[:n])
        rc = _lib.load().kzg_compute_quotient_eval_on_domain(ctx.handle, _lib.ptr(_lib.as_u64(z_fr, 0).reshape(4)), _lib.ptr(ev), n,
                                                             _lib.ptr(_lib.as_u64(value_fr, 0).reshape(4)), _lib.ptr(out))
        if rc == _lib.ERR_INVALID_ARG and not _lib.as_u64(z_fr, 0).any():
            raise ZeroDivisionError("compute_quotient_eval_on_domain: z = 0 (the reference divides by z)")
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return out

    # kzg.rs:263-285
    def g1_ifft(self, length: int, srs):
        """Lagrange-basis SRS of size `length` (natural order), (length, 8) uint64 wire points."""
        if length <= 0 or (length & (length - 1)) != 0:
            raise FFTError("length provided is not a power of 2")
        ctx = self._ctx()
        out = np.zeros((length, 8), dtype=np.uint64)
        rc = _lib.load().kzg_g1_ifft(ctx.handle, srs.handle, length, _lib.ptr(out))
        if rc == _lib.ERR_NOT_POWER_OF_TWO:
            raise FFTError("length provided is not a power of 2")
        if rc == _lib.ERR_DOMAIN:
            raise FFTError("Could not perform IFFT due to domain consturction error")
        if rc == _lib.ERR_SRS_CAPACITY_EXCEEDED:
            raise SrsCapacityExceeded(length, len(srs))
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return out

    # kzg.rs:288-309
    def compute_blob_proof(self, blob, commitment, srs, want_zy=False):
        """Bytes in, proof out (`kzg_compute_blob_proof`): commitment validation, Fiat-Shamir challenge (hashed in C on a host
        thread beside the upload) and the proof in one call."""
        ctx = self._ctx()
        data = blob.data()
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
        out = np.zeros(8, dtype=np.uint64); inf = C.c_uint8(0); z = np.zeros(4, dtype=np.uint64); y = np.zeros(4, dtype=np.uint64)
        rc = _lib.load().kzg_compute_blob_proof(ctx.handle, srs.handle, buf.ctypes.data_as(_lib.u8p), len(data), len(self.expanded_roots_of_unity),
                                                _lib.ptr(_lib.as_u64(commitment, 0).reshape(8)), _lib.ptr(out), C.byref(inf), _lib.ptr(z), _lib.ptr(y))
        self._raise_proof_status(ctx, rc, blob, srs)
        return (out, z, y) if want_zy else out

    def commit_and_prove_blob(self, blob, srs):
        """`commit_blob` + `compute_blob_proof` of the same blob in one call (`kzg_commit_and_prove_blob`): the transcript hash
        runs on a host thread while the GPU computes the commitment.  Returns (commitment, proof, z, y)."""
        ctx = self._ctx()
        data = blob.data()
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
        com = np.zeros(8, dtype=np.uint64); cinf = C.c_uint8(0)
        out = np.zeros(8, dtype=np.uint64); inf = C.c_uint8(0); z = np.zeros(4, dtype=np.uint64); y = np.zeros(4, dtype=np.uint64)
        rc = _lib.load().kzg_commit_and_prove_blob(ctx.handle, srs.handle, buf.ctypes.data_as(_lib.u8p), len(data), len(self.expanded_roots_of_unity),
                                                   _lib.ptr(com), C.byref(cinf), _lib.ptr(out), C.byref(inf), _lib.ptr(z), _lib.ptr(y))
        self._raise_proof_status(ctx, rc, blob, srs)
        return com, out, z, y

    # ---- the batched prover: many proofs in one call (no counterpart in the reference; same values as that many single calls) ----------
    def compute_proof_batch(self, polynomials, zs, srs, want_y=False):
        """`compute_proof` of every (polynomial, z) pair in ONE call (`kzg_compute_proof_batch`): `polynomials` is a list of
        PolynomialEvalForm of one length n (or a (count, n, 4) array of wire evaluations), `zs` one point per polynomial.  Returns a
        (count, 8) array of wire points (the identity as zeros), row b bit-identical to `compute_proof(polynomials[b], zs[b], srs)` on a
        KZG whose roots have that length; with want_y also the (count, 4) values f_b(z_b).  One fused kernel computes the values and the
        quotients (one workgroup per polynomial of up to 4 096 evaluations, points on the domain included), one batched MSM the proofs."""
        if isinstance(polynomials, np.ndarray):
            if polynomials.ndim != 3 or polynomials.shape[2] != 4:
                raise GenericError("compute_proof_batch takes a (count, n, 4) array")
            data = np.ascontiguousarray(polynomials, dtype=np.uint64)
            count, n = int(data.shape[0]), int(data.shape[1])
        else:
            rows = [_lib.as_u64(p.evaluations() if hasattr(p, "evaluations") else p, 4).reshape(-1, 4) for p in polynomials]
            count = len(rows)
            n = len(rows[0]) if rows else 0
            if any(len(r) != n for r in rows):
                raise GenericError("batched proofs need polynomials of one length")
            data = np.ascontiguousarray(np.stack(rows), dtype=np.uint64) if count and n else np.zeros((count, 0, 4), dtype=np.uint64)
        z = np.ascontiguousarray(np.stack([_lib.as_u64(v, 0).reshape(4) for v in zs]), dtype=np.uint64) if len(zs) else np.zeros((0, 4), dtype=np.uint64)
        if len(z) != count:
            raise GenericError("one point per polynomial")
        out = np.zeros((count, 8), dtype=np.uint64); inf = np.zeros(max(count, 1), dtype=np.uint8); y = np.zeros((count, 4), dtype=np.uint64)
        if count == 0:
            return (out, y) if want_y else out
        if n > len(srs):
            raise SrsCapacityExceeded(n, len(srs))
        ctx = self._ctx()
        rc = _lib.load().kzg_compute_proof_batch(ctx.handle, srs.handle, _lib.ptr(data) if data.size else None, n, count, _lib.ptr(z), _lib.ptr(out),
                                                 inf.ctypes.data_as(_lib.u8p), _lib.ptr(y))
        if rc == _lib.ERR_SRS_CAPACITY_EXCEEDED:
            raise SrsCapacityExceeded(n, len(srs))
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return (out, y) if want_y else out

    def _blob_proof_batch(self, blobs, commitments, srs):
        ctx = self._ctx()
        blobs = list(blobs)
        count = len(blobs)
        ptrs, lens, keep = _lib.blob_args(blobs)
        com = np.zeros((count, 8), dtype=np.uint64); out = np.zeros((count, 8), dtype=np.uint64); inf = np.zeros(max(count, 1), dtype=np.uint8)
        z = np.zeros((count, 4), dtype=np.uint64); y = np.zeros((count, 4), dtype=np.uint64)
        bad = C.c_size_t(0)
        lib = _lib.load()
        if commitments is None:
            rc = lib.kzg_commit_and_prove_blob_batch(ctx.handle, srs.handle, ptrs, lens, count, _lib.ptr(com), None, _lib.ptr(out), inf.ctypes.data_as(_lib.u8p),
                                                     _lib.ptr(z), _lib.ptr(y), C.byref(bad))
        else:
            rows = [_lib.as_u64(c, 0).reshape(8) for c in commitments]
            if len(rows) != count:
                raise GenericError("one commitment per blob")
            com = np.ascontiguousarray(np.stack(rows), dtype=np.uint64) if count else com
            rc = lib.kzg_compute_blob_proof_batch(ctx.handle, srs.handle, ptrs, lens, _lib.ptr(com), count, _lib.ptr(out), inf.ctypes.data_as(_lib.u8p), _lib.ptr(z),
                                                  _lib.ptr(y), C.byref(bad))
        del keep
        if rc != _lib.OK:
            self._raise_proof_status(ctx, rc, blobs[bad.value] if bad.value < count else blobs[0], srs)
        return com, out, z, y

    def compute_blob_proof_batch(self, blobs, commitments, srs, want_zy=False):
        """`compute_blob_proof` of every (blob, commitment) pair in ONE call (`kzg_compute_blob_proof_batch`), the blobs of any mix of
        lengths: a (count, 8) array of proofs, row b bit-identical to `compute_blob_proof(blobs[b], commitments[b], srs)`; with want_zy also
        the (count, 4) challenges and values.  Raises what the single method raises, for the first failing blob in index order."""
        _, out, z, y = self._blob_proof_batch(blobs, list(commitments), srs)
        return (out, z, y) if want_zy else out

    def commit_and_prove_blob_batch(self, blobs, srs):
        """`commit_and_prove_blob` of every blob in ONE call (`kzg_commit_and_prove_blob_batch`): (commitments (count, 8), proofs (count, 8),
        zs (count, 4), ys (count, 4)), row b bit-identical to the single method on blobs[b] -- what `verifier.verify_blob_kzg_proof_batch`
        takes."""
        return self._blob_proof_batch(blobs, None, srs)

    # the same as a stream (`kzg_commit_and_prove_blob_begin` / `_end`): up to _lib.BLOB_JOBS blobs in flight, their transcript hashes side by side
    def commit_and_prove_blob_begin(self, blob, srs, job, commitment=None):
        """Starts job `job` (0 .. BLOB_JOBS-1): the transcript prefix on a host thread of the library, upload + bytes -> Fr + commitment on the
        GPU; returns at once.  `commitment` given: `compute_blob_proof` as it stands (validated, absorbed, not recomputed).  The blob's bytes are
        kept alive here until the job's end call."""
        ctx = self._ctx()
        data = blob.data()
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
        cptr = _lib.ptr(_lib.as_u64(commitment, 0).reshape(8)) if commitment is not None else None
        rc = _lib.load().kzg_commit_and_prove_blob_begin(ctx.handle, srs.handle, buf.ctypes.data_as(_lib.u8p), len(data), len(self.expanded_roots_of_unity),
                                                         cptr, job)
        self._raise_proof_status(ctx, rc, blob, srs)
        if not hasattr(self, "_blob_jobs"):
            self._blob_jobs = {}
        self._blob_jobs[job] = (buf, data, blob, srs)

    def commit_and_prove_blob_end(self, job):
        """(commitment, proof, z, y) of job `job`; waits for what is still missing and moves the other jobs on meanwhile."""
        ctx = self._ctx()
        com = np.zeros(8, dtype=np.uint64); cinf = C.c_uint8(0)
        out = np.zeros(8, dtype=np.uint64); inf = C.c_uint8(0); z = np.zeros(4, dtype=np.uint64); y = np.zeros(4, dtype=np.uint64)
        rc = _lib.load().kzg_commit_and_prove_blob_end(ctx.handle, job, _lib.ptr(com), C.byref(cinf), _lib.ptr(out), C.byref(inf), _lib.ptr(z), _lib.ptr(y))
        held = getattr(self, "_blob_jobs", {}).pop(job, None)
        if rc != _lib.OK and held is not None:
            self._raise_proof_status(ctx, rc, held[2], held[3])
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(ctx.last_error() or _lib.status_message(rc))
        return com, out, z, y

    def commit_and_prove_blobs(self, blobs, srs, inflight=8):
        """Generator over an iterable of blobs: yields (commitment, proof, z, y) per blob, in order, with `inflight` jobs in flight."""
        inflight = max(1, min(int(inflight), _lib.BLOB_JOBS))
        pending = []                                   # job indices in begin order
        free = list(range(inflight))
        try:
            for blob in blobs:
                if not free:
                    j = pending.pop(0)
                    res = self.commit_and_prove_blob_end(j)
                    free.append(j)
                    yield res
                j = free.pop(0)
                self.commit_and_prove_blob_begin(blob, srs, j)
                pending.append(j)
            while pending:
                j = pending.pop(0)
                res = self.commit_and_prove_blob_end(j)
                free.append(j)
                yield res
        finally:
            for j in pending:                          # (an exception or an abandoned generator: nothing stays in flight)
                try:
                    self.commit_and_prove_blob_end(j)
                except Exception:
                    pass

    @staticmethod
    def _raise_proof_status(ctx, rc, blob, srs):
        if rc == _lib.OK:
            return
        if rc == _lib.ERR_G1_NOT_ON_CURVE:
            raise NotOnCurveError("G1 point not on curve")
        if rc == _lib.ERR_ROOTS_LENGTH:
            raise GenericError("inconsistent length between blob and root of unities")
        if rc == _lib.ERR_SRS_CAPACITY_EXCEEDED:
            raise SrsCapacityExceeded(-(-len(blob.data()) // 32), len(srs))
        if rc == _lib.ERR_TOO_LARGE:
            raise GenericError("Input size exceeds maximum polynomial size")
        ctx.check_device(rc)
        raise GenericError(_lib.status_message(rc))
