"""G2 powers of tau RESIDENT ON THE GPU (`kzg_g2srs` of the C-ABI, 128 B per point): the bases of the protocol's length commitment
sum f_i [tau^i]_2 and length proof sum f_i [tau^(N-d+i)]_2 (`KZG.commit_with_length_proof`), and of any G2 MSM (`helpers.msm_g2` takes
caller bases instead)."""
import ctypes as C

import numpy as np

from . import _lib
from .errors import DeserializationError, GenericError, NotOnCurveError
from .fr import fr_from_int


class G2SRS:
    def __init__(self, handle, n, ctx, first_power=0):
        self.ctx, self.handle, self._n, self.first_power = ctx, handle, int(n), int(first_power)

    @classmethod
    def generate(cls, tau: int, n: int, first_power: int = 0, ctx=None):
        """[tau^(first_power + i)]_2 for i < n and a known tau, computed on the device (`kzg_g2srs_generate`; tests, custom setups)."""
        ctx = ctx or _lib.default_context()
        h = C.c_void_p()
        rc = _lib.load().kzg_g2srs_generate(ctx.handle, _lib.ptr(fr_from_int(tau)), first_power, n, C.byref(h))
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return cls(h, n, ctx, first_power)

    @classmethod
    def from_points(cls, wire, first_power: int = 0, ctx=None):
        """(n, 16) uint64 wire points -> device (`kzg_g2srs_upload`): every point is checked on the twist there (the subgroup is not)."""
        ctx = ctx or _lib.default_context()
        pts = np.ascontiguousarray(_lib.as_u64(wire, 16)).reshape(-1, 16)
        h = C.c_void_p()
        bad = C.c_uint64(0)
        rc = _lib.load().kzg_g2srs_upload(ctx.handle, _lib.ptr(pts) if len(pts) else None, len(pts), C.byref(h), C.byref(bad))
        if rc == _lib.ERR_NOT_ON_CURVE:
            raise NotOnCurveError("G2 point %d not on curve" % bad.value)
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return cls(h, len(pts), ctx, first_power)

    @staticmethod
    def decompress(data: bytes) -> np.ndarray:
        """gnark-compressed G2 points (64 bytes each) -> (n, 16) wire points (`kzg_g2_decompress_be`, host)."""
        if len(data) == 0 or len(data) % 64 != 0:
            raise DeserializationError("a file of compressed G2 points is a positive multiple of 64 bytes")
        n = len(data) // 64
        out = np.zeros((n, 16), dtype=np.uint64)
        bad = C.c_uint64(0)
        buf = np.frombuffer(data, dtype=np.uint8)
        rc = _lib.load().kzg_g2_decompress_be(buf.ctypes.data_as(_lib.u8p), n, _lib.ptr(out), C.byref(bad))
        if rc == _lib.ERR_DESERIALIZE:
            raise DeserializationError("G2 point %d: not a compressed finite point below the modulus" % bad.value)
        if rc == _lib.ERR_NOT_ON_CURVE:
            raise NotOnCurveError("G2 point %d not on curve or not in the correct subgroup" % bad.value)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return out

    @staticmethod
    def _check_decoded(rc, bad, ctx):
        if rc == _lib.ERR_DESERIALIZE:
            raise DeserializationError("G2 point %d: not a compressed finite point below the modulus" % bad)
        if rc == _lib.ERR_NOT_ON_CURVE:
            raise NotOnCurveError("G2 point %d not on curve or not in the correct subgroup" % bad)
        ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))

    @staticmethod
    def decompress_device(data: bytes, check_subgroup: bool = True, reject_generator: bool = True, ctx=None) -> np.ndarray:
        """gnark-compressed G2 points (64 bytes each) -> (n, 16) wire points, decoded on the GPU (`kzg_g2_decompress_be_device`).  With both
        checks: the points, the exception and its index are those of `decompress`; with neither: only "on the twist"."""
        if len(data) == 0 or len(data) % 64 != 0:
            raise DeserializationError("a file of compressed G2 points is a positive multiple of 64 bytes")
        ctx = ctx or _lib.default_context()
        n = len(data) // 64
        out = np.zeros((n, 16), dtype=np.uint64)
        bad = C.c_uint64(0)
        buf = np.frombuffer(data, dtype=np.uint8)
        flags = (_lib.G2_CHECK_SUBGROUP if check_subgroup else 0) | (_lib.G2_REJECT_GENERATOR if reject_generator else 0)
        rc = _lib.load().kzg_g2_decompress_be_device(ctx.handle, buf.ctypes.data_as(_lib.u8p), n, flags, _lib.ptr(out), C.byref(bad))
        G2SRS._check_decoded(rc, bad.value, ctx)
        return out

    @classmethod
    def from_file(cls, path, points_to_load: int, first_power: int = 0, ctx=None, offset_points: int = 0):
        """`points_to_load` gnark-compressed points of a file, from point `offset_points` on (a disperser loads the trailing window
        [tau^(N-d) ..]_2 of the same file), decoded and subgroup-checked on the GPU straight into the handle
        (`kzg_g2srs_load_compressed_be`).  The generator is accepted: a file of powers of tau starts with [tau^0]_2."""
        ctx = ctx or _lib.default_context()
        with open(path, "rb") as f:
            f.seek(64 * offset_points)
            data = f.read(64 * points_to_load)
        if len(data) != 64 * points_to_load:
            raise GenericError(f"Expected {points_to_load} points, only read {len(data) // 64}")
        if len(data) == 0:
            raise DeserializationError("a file of compressed G2 points is a positive multiple of 64 bytes")
        h = C.c_void_p()
        bad = C.c_uint64(0)
        buf = np.frombuffer(data, dtype=np.uint8)
        rc = _lib.load().kzg_g2srs_load_compressed_be(ctx.handle, buf.ctypes.data_as(_lib.u8p), points_to_load, C.byref(h), C.byref(bad))
        cls._check_decoded(rc, bad.value, ctx)
        return cls(h, points_to_load, ctx, first_power)

    @property
    def g2(self):
        """The points, read back from the device in wire format."""
        out = np.zeros((self._n, 16), dtype=np.uint64)
        if self._n:
            self.ctx.check_device(_lib.load().kzg_g2srs_download(self.ctx.handle, self.handle, 0, self._n, _lib.ptr(out)))
        return out

    def msm_batch(self, scalars, offset: int = 0) -> np.ndarray:
        """(B, n, 4) Fr wire scalars -> (B, 16) wire points: row b = sum_i scalars[b][i] * point[offset + i] (`kzg_msm_g2_srs_batch`), the
        blobs of a group in one sort and one launch sequence; bit for bit the single MSM of every row."""
        sc = np.ascontiguousarray(scalars, dtype=np.uint64)
        if sc.ndim != 3 or sc.shape[2] != 4:
            raise GenericError("scalars: a (B, n, 4) array of Fr wire words")
        count, n = sc.shape[0], sc.shape[1]
        out = np.zeros((count, 16), dtype=np.uint64)
        rc = _lib.load().kzg_msm_g2_srs_batch(self.ctx.handle, self.handle, offset, _lib.ptr(sc) if sc.size else None, n, count, _lib.ptr(out), None)
        if rc == _lib.ERR_POLY_LENGTH:
            raise GenericError("polynomial length is not correct")
        self.ctx.check_device(rc)
        if rc != _lib.OK:
            raise GenericError(_lib.status_message(rc))
        return out

    def __len__(self):
        return self._n

    def close(self):
        if getattr(self, "handle", None):
            _lib.load().kzg_g2srs_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
