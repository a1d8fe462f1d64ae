"""Big-integer arithmetic on BN254's twist E': y^2 = x^3 + 3 / (9 + u) over Fq2 = Fq[u] / (u^2 + 1), for tests that need points OUTSIDE
the order-r subgroup (the library's own entries only make multiples of the generator).  Points are ((x0, x1), (y0, y1)) or None for
the identity.  #E' = r (2p - r); 2p - r = 10069 * 5864401 * (a large cofactor)."""
import numpy as np

import pyref
from pyref import P, R_

COFACTOR = 2 * P - R_
ORDER = R_ * COFACTOR
SMALL_FACTORS = (10069, 5864401)
assert COFACTOR % SMALL_FACTORS[0] == 0 and COFACTOR % SMALL_FACTORS[1] == 0

_D = pow(82, P - 2, P)
B = (27 * _D % P, -3 * _D % P)                      # 3 / (9 + u)


def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2inv(a):
    n = pow((a[0] * a[0] + a[1] * a[1]) % P, P - 2, P)
    return (a[0] * n % P, -a[1] * n % P)


def f2sqrt(a):
    """sqrt in Fq2 (p = 3 mod 4); None when there is none"""
    a0, a1 = a
    if a1 == 0:
        s = pow(a0, (P + 1) // 4, P)
        if s * s % P == a0:
            return s, 0
        s = pow(-a0 % P, (P + 1) // 4, P)
        return (0, s) if s * s % P == -a0 % P else None
    norm = (a0 * a0 + a1 * a1) % P
    s = pow(norm, (P + 1) // 4, P)
    if s * s % P != norm:
        return None
    inv2 = pow(2, P - 2, P)
    for cand in ((a0 + s) * inv2 % P, (a0 - s) * inv2 % P):
        x0 = pow(cand, (P + 1) // 4, P)
        if x0 and x0 * x0 % P == cand:
            return x0, a1 * pow(2 * x0, P - 2, P) % P
    return None


def on_twist(pt):
    if pt is None:
        return True
    x, y = pt
    return f2mul(y, y) == f2add(f2mul(f2mul(x, x), x), B)


def add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if a[1] != b[1] or a[1] == (0, 0):
            return None
        xx = f2mul(a[0], a[0])
        lam = f2mul(f2add(f2add(xx, xx), xx), f2inv(f2add(a[1], a[1])))
    else:
        lam = f2mul(f2sub(b[1], a[1]), f2inv(f2sub(b[0], a[0])))
    x3 = f2sub(f2sub(f2mul(lam, lam), a[0]), b[0])
    return x3, f2sub(f2mul(lam, f2sub(a[0], x3)), a[1])


def neg(a):
    return None if a is None else (a[0], ((-a[1][0]) % P, (-a[1][1]) % P))


def mul(k, a):
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, a)
    return acc


def random_twist_point(rng):
    """a random point of E'(Fq2) by the square-root construction: outside the subgroup with probability 1 - 1 / (2p - r)"""
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        y = f2sqrt(f2add(f2mul(f2mul(x, x), x), B))
        if y is not None:
            return x, y


def point_of_order(f, rng):
    """a point of prime order f | 2p - r: [#E' / f]Q for random Q until it is not the identity"""
    while True:
        pt = mul(ORDER // f, random_twist_point(rng))
        if pt is not None:
            assert mul(f, pt) is None
            return pt


def to_wire(pt):
    """16 u64: x.c0 | x.c1 | y.c0 | y.c1 in Montgomery form; the identity is all zero"""
    if pt is None:
        return np.zeros(16, np.uint64)
    return np.concatenate([pyref.fq_to_mont(v) for v in (pt[0][0], pt[0][1], pt[1][0], pt[1][1])])


def from_wire(w):
    w = np.asarray(w, np.uint64).reshape(16)
    if not w.any():
        return None
    v = [pyref.fq_from_mont(w[4 * j:4 * j + 4]) for j in range(4)]
    return (v[0], v[1]), (v[2], v[3])
