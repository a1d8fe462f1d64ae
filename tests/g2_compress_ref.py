"""Python integers: G2 points -> the gnark compression that `helpers.read_g2_powers_of_2`, `kzg_g2_decompress_be` and the device decoder
read (64 bytes: X.A1 || X.A0 big-endian, the top two bits of the first byte 0b10 = the smaller y, 0b11 = the larger, "larger" on
(y.c1, y.c0) against (p - 1) / 2).  The GPU tests of the device decoder make their inputs with it."""
import numpy as np

import g2_points
from pyref import P

HALF = (P - 1) // 2


def is_largest(y) -> bool:
    """gnark's LexicographicallyLargest of y = (y0, y1)"""
    return y[1] > HALF if y[1] else y[0] > HALF


def compress_point(pt, negate=False) -> bytes:
    """((x0, x1), (y0, y1)) -> 64 bytes; negate: the bytes of -pt (the same x with the other flag)"""
    (x0, x1), y = pt
    flag = 3 if is_largest(y) != bool(negate) else 2
    if y == (0, 0):
        flag = 2
    b = bytearray(x1.to_bytes(32, "big") + x0.to_bytes(32, "big"))
    b[0] |= flag << 6
    return bytes(b)


def compress_x(x, flag) -> bytes:
    """an x = (x0, x1) with explicit flag bits"""
    b = bytearray(x[1].to_bytes(32, "big") + x[0].to_bytes(32, "big"))
    b[0] |= flag << 6
    return bytes(b)


def compress_wire(wire, negate=False) -> bytes:
    """(n, 16) uint64 wire points (none the identity) -> 64 n bytes"""
    pts = np.ascontiguousarray(wire, dtype=np.uint64).reshape(-1, 16)
    return b"".join(compress_point(g2_points.from_wire(w), negate) for w in pts)


def negate_wire(wire) -> np.ndarray:
    """the wire points with every y negated"""
    pts = np.ascontiguousarray(wire, dtype=np.uint64).reshape(-1, 16)
    return np.stack([g2_points.to_wire(g2_points.neg(g2_points.from_wire(w))) for w in pts])
