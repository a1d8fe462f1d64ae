"""Plain-integer restatement of the GLV decomposition of csrc/glv.h, for tests/test_glv_host.py and tests/test_gpu_glv.py.

The six constant arrays are read out of the header itself, so a changed constant is a changed test input.  decompose(k) is the
header's rule word for word (c1 = k g1 >> 256, c2 = k g2 >> 256, k1 = k - c1 a1 - c2 a2, k2 = c1 |b1| - c2 b2) and returns the
eight words glv_decompose writes; halves_value(kk) is the scalar those words stand for, +-|k1| +- |k2| lambda mod r.
"""
import os
import random
import re

from pyref import P, R_

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rust-kzg-bn254_amd", "csrc", "glv.h")
LENGTHS = {"G1": 3, "G2": 5, "A1": 2, "B1M": 4, "A2": 4, "BETA": 8}


def read_constants(path=HEADER):
    """{name: int} of the GLV_* word arrays of the header (little-endian 32-bit words)"""
    text = open(path).read()
    out = {}
    for name, n, body in re.findall(r"static\s+__device__\s+const\s+uint32_t\s+GLV_(\w+)\[(\d+)\]\s*=\s*\{([^}]*)\}", text):
        words = [int(w.strip().rstrip("uU"), 16) for w in body.split(",") if w.strip()]
        assert len(words) == int(n) == LENGTHS[name], (name, n, words)
        assert all(0 <= w < 1 << 32 for w in words)
        out[name] = sum(w << (32 * j) for j, w in enumerate(words))
    assert set(out) == set(LENGTHS), sorted(out)
    return out


_C = read_constants()
G1, G2, A1, B1M, A2, BETA = (_C[n] for n in ("G1", "G2", "A1", "B1M", "A2", "BETA"))
B2 = A1                                          # the header's b2 = a1;  b1 = -B1M
LAMBDA = A1 * pow(B1M, -1, R_) % R_              # -a1 / b1 mod r
HALF = 1 << 127                                  # the chains read 127 bits of each half
SIGN = 1 << 31


def split(k):
    """(k1, k2) as signed integers"""
    c1, c2 = (k * G1) >> 256, (k * G2) >> 256
    return k - c1 * A1 - c2 * A2, c1 * B1M - c2 * B2


def pack(k1, k2):
    """signed halves -> the eight words: the low 128 bits of each magnitude, the sign in bit 31 of words 3 and 7 (as the device, which
    takes the low four words of a 256-bit magnitude: a half of 2^127 or more would come out wrong here exactly as it would there)"""
    words = []
    for h in (k1, k2):
        mag = abs(h) & ((1 << 128) - 1)
        w = [(mag >> (32 * j)) & 0xFFFFFFFF for j in range(4)]
        if h < 0:
            w[3] |= SIGN
        words += w
    return words


def decompose(k):
    assert 0 <= k < R_
    return pack(*split(k))


def unpack(kk):
    """eight words -> (k1, k2) as signed integers: 127-bit magnitudes, signs from bit 31 of words 3 and 7"""
    halves = []
    for base in (0, 4):
        mag = sum(int(kk[base + j]) << (32 * j) for j in range(4)) & (HALF - 1)
        halves.append(-mag if int(kk[base + 3]) & SIGN else mag)
    return tuple(halves)


def halves_value(kk):
    k1, k2 = unpack(kk)
    return (k1 + k2 * LAMBDA) % R_


# ----- the scalars of the decomposition tests ------------------------------------------------------------------------------------
def boundary(c, g):
    """the largest k with floor(k g / 2^256) < c: its quotient c - 1 has the largest fractional part left behind"""
    return -((-c << 256) // g) - 1


def search_extremes(rnd, tries=4000):
    """(k with the largest |k2|, k with the largest |k1|) among the floor boundaries.  g1 is rounded down, so k g1 / 2^256 falls short of
    k b2 / r by up to e1 k / r and |k2| peaks at the boundaries of g1 with the quotient in the top 2 % of its range (k near r); g2 is
    rounded up, so |k1| peaks where that excess is smallest: the boundaries of g2 with a small quotient, where it comes to a2 almost exactly."""
    cmax1, cmax2 = ((R_ - 1) * G1) >> 256, ((R_ - 1) * G2) >> 256
    ks2 = [boundary(cmax1 - rnd.randrange(cmax1 // 50), G1) for _ in range(tries)] + [boundary(cmax1 - j, G1) for j in range(64)]
    ks1 = [boundary(rnd.randrange(1, cmax2), G2) for _ in range(tries)] + [boundary(c, G2) for c in range(1, 65)]
    return (max((k for k in ks2 if 0 <= k < R_), key=lambda k: abs(split(k)[1])),
            max((k for k in ks1 if 0 <= k < R_), key=lambda k: abs(split(k)[0])))


K2_EXTREME = 0x30644e1a4d7a33b8b20680a578b2ce9067544f5b7d240c6cd2a77771c2cfd9d4   # |k2| = 0.94064745 2^127


def scalar_groups(seed=20240127):
    """{name: [k, ...]}: every scalar of the decomposition tests, by the reason it is there"""
    rnd = random.Random(seed)
    lam = LAMBDA
    g = {}
    g["edges"] = [0, 1, 2, R_ - 1, R_ - 2, (R_ + 1) // 2, (R_ - 1) // 2, lam, lam + 1, lam - 1, lam * lam % R_, R_ - lam,
                  (1 << 64) - 1, 1 << 64, (1 << 127) - 1, 1 << 127, 1 << 128, 1 << 253]
    g["small"] = [rnd.randrange(1 << 64) for _ in range(50)]
    g["lambda_multiples"] = [rnd.randrange(1 << 100) * lam % R_ for _ in range(50)]
    g["random"] = [rnd.randrange(R_) for _ in range(2000)]
    floors = []
    for gg in (G1, G2):
        cmax = ((R_ - 1) * gg) >> 256
        for _ in range(50):
            k0 = boundary(rnd.randrange(2, cmax), gg)
            floors += [k0 - 1, k0, k0 + 1]
    g["floor_boundaries"] = floors
    k2x, k1x = search_extremes(rnd)
    g["extremes"] = [K2_EXTREME, k2x, k1x]
    for name, ks in g.items():
        assert all(0 <= k < R_ for k in ks), name
    return g


def scalars(seed=20240127):
    return [k for ks in scalar_groups(seed).values() for k in ks]


__all__ = ["P", "R_", "G1", "G2", "A1", "A2", "B1M", "B2", "BETA", "LAMBDA", "HALF", "split", "pack", "decompose", "unpack", "halves_value",
           "boundary", "search_extremes", "scalar_groups", "scalars", "read_constants", "K2_EXTREME"]
