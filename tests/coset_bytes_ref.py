"""Big-integer twin of the serialized form of coset items (tests only): gnark-compressed G1 points and big-endian scalars, the strict
decode rules of csrc/g1_decode.h, written independently of the library."""
from pyref import P, R_

KIND_DESERIALIZE, KIND_NOT_ON_CURVE, KIND_OK, KIND_IDENTITY = 0, 1, 4, 5
IDENTITY_BE = b"\x40" + bytes(31)


def compress_be(pt) -> bytes:
    """(x, y) or None -> 32 bytes: x big-endian, 0b10 / 0b11 in the top two bits of byte 0 for the smaller / larger y"""
    if pt is None:
        return IDENTITY_BE
    b = bytearray(pt[0].to_bytes(32, "big"))
    b[0] |= 0xC0 if pt[1] > (P - 1) // 2 else 0x80
    return bytes(b)


def decode_be(b: bytes):
    """32 bytes -> (kind, point or None) by the strict rules, in their order"""
    flag = b[0] >> 6
    if flag == 0:
        return KIND_DESERIALIZE, None
    rest = int.from_bytes(bytes([b[0] & 0x3F]) + b[1:], "big")
    if flag == 1:
        return (KIND_DESERIALIZE, None) if rest else (KIND_IDENTITY, None)
    if rest >= P:
        return KIND_DESERIALIZE, None
    y2 = (rest * rest * rest + 3) % P
    y = pow(y2, (P + 1) // 4, P)
    if y * y % P != y2:
        return KIND_NOT_ON_CURVE, None
    if (y > (P - 1) // 2) != (flag == 3):
        y = P - y
    return KIND_OK, (rest, y)


def record(b: bytes) -> bytes:
    """the record tests/hostcheck/g1decodecheck.cpp reads: input, expected kind, expected x || y"""
    kind, pt = decode_be(b)
    xy = pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big") if pt else bytes(64)
    return bytes(b) + bytes([kind]) + xy


def x_without_point(x: int) -> int:
    """the first x' >= x with no point on the curve"""
    while True:
        y2 = (x * x * x + 3) % P
        if pow(y2, (P - 1) // 2, P) != 1 and y2 != 0:
            return x
        x += 1


def values_be(vals) -> bytes:
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


__all__ = ["P", "R_", "compress_be", "decode_be", "record", "x_without_point", "values_be", "IDENTITY_BE", "KIND_DESERIALIZE", "KIND_NOT_ON_CURVE", "KIND_OK",
           "KIND_IDENTITY"]
