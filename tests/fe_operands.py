"""Operand sets and big-integer expectations for the field primitives of csrc/field29.h / fe_invert.h, shared by the host test of the
bound predicates (test_field29_bounds_host.py) and the device conformance test (test_gpu_device_math.py).

An operand row is 36 int32: the raw signed limbs of a, b, c, d (9 each, value sum l_j 2^(29 j)); wire words travel in the first 8
limbs of a.  A result row is 18 int32: r and s.  The op numbers mirror enum DcOp of tests/devcheck/dc_prims.h.

The sets aim at the edges of the lazy formulas: limb products and values just under the bounds the headers state (both at once too),
canonical edges, the (-6m, 9m) ranges curve.h annotates, and many random legal operands.
"""
import random

import numpy as np

from pyref import P, R_

NL, LB = 9, 29
MASK = (1 << LB) - 1
MODS = {0: P, 1: R_}
RADIX = 1 << 261

(MUL, SQR, MUL2, SQR2, MULSUB, MUL_ILP, ADD, SUB, DBL, NORM, CANON, IS_ZERO_MOD, REDUCE, REDUCE_SMALL, FROM_WIRE, TO_WIRE,
 WIRE_TO_CANONICAL, INVERT) = range(18)
NAMES = ["fe_mul", "fe_sqr", "fe_mul2", "fe_sqr2", "fe_mulsub", "fe_mul_ilp", "fe_add", "fe_sub", "fe_dbl", "fe_norm", "fe_canon",
         "fe_is_zero_mod", "fe_reduce", "fe_reduce_small", "fe_from_wire", "fe_to_wire", "fe_wire_to_canonical_words", "fe_invert"]
PRODUCTS = (MUL, SQR, MUL2, SQR2, MULSUB, MUL_ILP)

MUL_LIMB_LIMIT = 7.3e17                       # field29.h KZG_MUL_LIMB_LIMIT: max|a_j| max|b_j| (2^59.35 = 7.366e17 with margin)
MULSUB_LIMB_LIMIT = (2 ** 63 - 1 - 9 * 2 ** 58) / 9     # max|a||b| + max|c||d| (27 * 2^58 per column with limbs at 2^29)
REDUCE_LIMIT = 169


# ----- limbs <-> integers ------------------------------------------------------------------------------------------------------------
def limbs(v):
    """normalised limbs of the integer v: l_0..l_7 in [0, 2^29), l_8 signed"""
    return [(v >> (LB * j)) & MASK for j in range(NL - 1)] + [v >> (LB * (NL - 1))]


def value(l):
    return sum(int(x) << (LB * j) for j, x in enumerate(l))


def values(arr, slot=0):
    """big-integer values of slot `slot` (0..3) of every row of an (n, 36) or (n, 18) int32 array"""
    a = np.asarray(arr, dtype=np.int64)[:, NL * slot:NL * slot + NL]
    return [sum(int(x) << (LB * j) for j, x in enumerate(row)) for row in a.tolist()]


def words_value(row):
    return sum((int(x) & 0xFFFFFFFF) << (32 * j) for j, x in enumerate(row[:8]))


def value_words(v):
    """the 8 little-endian u32 words of v as int32 limbs of a slot"""
    return [((v >> (32 * j)) & 0xFFFFFFFF) - ((v >> (32 * j + 31) & 1) << 32) for j in range(8)] + [0]


def normalised(l):
    return all(0 <= int(x) <= MASK for x in l[:NL - 1])


def max_limb(l):
    return max(abs(int(x)) for x in l)


def row(*ops):
    out = []
    for k in range(4):
        out += list(ops[k]) if k < len(ops) else [0] * NL
    return out


def to_array(rows):
    a = np.array(rows, dtype=np.int64)
    assert a.size == 0 or (a.min() >= -(1 << 31) and a.max() < (1 << 31)), "an operand limb outside int32"
    return a.astype(np.int32)


# ----- the bounds, exactly (the C predicates evaluate the same in double) --------------------------------------------------------
def legal_mul(a, b, m):
    return float(max_limb(a)) * float(max_limb(b)) < MUL_LIMB_LIMIT and abs(value(a) * value(b)) < RADIX * m


def legal_mulsub(a, b, c, d, m):
    lim = float(max_limb(a)) * float(max_limb(b)) + float(max_limb(c)) * float(max_limb(d))
    return 9.0 * lim + 9.0 * 2.0 ** 58 < 2.0 ** 63 and abs(value(a) * value(b)) + abs(value(c) * value(d)) < RADIX * m


# ----- operand patterns ----------------------------------------------------------------------------------------------------------
TOP = (1 << 29) - 1


def extreme_patterns(rnd):
    """the signed limb patterns of test_field29_host.py::test_paired_multiplies_equal_the_single_forms_on_extreme_limbs"""
    hi = 1 << 22
    pats = [[TOP] * 8 + [hi], [-TOP] * 8 + [-hi], [TOP if j % 2 else -TOP for j in range(8)] + [hi],
            [-TOP if j % 2 else TOP for j in range(8)] + [-hi], [0] * 9, [1] + [0] * 8, [0] * 8 + [-(1 << 21)], [TOP] + [0] * 8,
            [0] * 8 + [hi], [-1] * 9]
    pats += [[rnd.randrange(-TOP, TOP + 1) for _ in range(8)] + [rnd.randrange(-hi, hi + 1)] for _ in range(40)]
    return pats


def canonical_edges(m):
    vs = [0, 1, 2, m - 1, m, m + 1, 2 * m - 1, -m + 1, -1, (m - 1) // 2, (m + 1) // 2, (1 << 232) - 1, (1 << 29) - 1, (1 << 58) - 1,
          (1 << 253) - 1, RADIX % m, (1 << 256) % m]
    vs += [1 << k for k in (0, 1, 28, 29, 30, 57, 58, 116, 231, 232, 233, 252, 253)]
    vs += [m - (1 << k) for k in (0, 29, 58, 232)]
    return vs


def lazy_values(m, rnd, n):
    """values in the lazy ranges curve.h annotates: (-6m, 9m), (-7m, 5m), (-4m, 5m), |.| < 6m ..."""
    out = [k * m + e for k in range(-6, 9) for e in (-1, 0, 1)]
    for lo, hi in ((-6, 9), (-7, 5), (-4, 5), (-6, 6), (-3, 3), (-1, 2)):
        out += [rnd.randrange(lo * m + 1, hi * m) for _ in range(n)]
    return out


def unnormalise(l, rnd, bound=1 << 29):
    """another limb representation of the same value (carries moved between limbs), every limb kept within +-bound"""
    l = list(l)
    for j in range(NL - 1):
        k = rnd.choice((-1, 0, 1))
        if abs(l[j] + (k << LB)) < bound and abs(l[j + 1] - k) < bound:
            l[j] += k << LB
            l[j + 1] -= k
    return l


def _signed_limbs(rnd, L, top):
    """limbs 0..7 of magnitude <= L with one of them exactly +-L, the given top limb"""
    l = [rnd.randrange(-L, L + 1) for _ in range(NL - 1)]
    l[rnd.randrange(NL - 1)] = L if rnd.randrange(2) else -L
    return l + [top]


def _with_value(rnd, L, target):
    """limbs 0..7 at +-L (mostly the sign of target) and the top limb chosen so that the value is close to target"""
    s = 1 if target >= 0 else -1
    low = [s * L if rnd.random() < 0.8 else rnd.randrange(-L, L + 1) for _ in range(NL - 1)]
    low[rnd.randrange(NL - 1)] = s * L
    lv = value(low + [0])
    top = (target - lv) >> (LB * (NL - 1))
    return low + [top]


def saturating_mul_pairs(m, rnd, n):
    """(a, b) pairs at the bounds of fe_mul: limbs only (max|a_j| max|b_j| in [0.99, 1) of the limit), value only (|a b| in [0.99, 1)
    of 2^261 m), both at once; every pair legal (checked exactly)."""
    T = RADIX * m
    out = []
    while len(out) < n:
        kind = len(out) % 3
        f = rnd.uniform(0.99, 0.9999)
        if kind == 0:                                   # limb bound alone: small top limbs keep the value far below its bound
            La = int(2 ** rnd.uniform(28.4, 30.6))
            Lb = int(f * MUL_LIMB_LIMIT / La)
            a = _signed_limbs(rnd, La, rnd.randrange(-(1 << 20), 1 << 20))
            b = _signed_limbs(rnd, Lb, rnd.randrange(-(1 << 20), 1 << 20))
        elif kind == 1:                                 # value bound alone: normalised limbs (< 2^29), tops ~2^25
            A = int(2 ** rnd.uniform(255.0, 259.5)) + rnd.getrandbits(230)
            a = limbs(A if rnd.randrange(2) else -A)
            B = int(f * T) // A
            b = limbs(B if rnd.randrange(2) else -B)
        else:                                           # both: low limbs at +-L with L^2 = f limit, values at f' 2^261 m
            L = int((f * MUL_LIMB_LIMIT) ** 0.5)
            A = int(2 ** rnd.uniform(256.5, 258.0)) * (1 if rnd.randrange(2) else -1)
            a = _with_value(rnd, L, A)
            B = int(rnd.uniform(0.99, 0.9999) * T) // abs(value(a)) * (1 if rnd.randrange(2) else -1)
            b = _with_value(rnd, L, B)
        if legal_mul(a, b, m):
            out.append((a, b))
    return out


def saturating_squares(m, rnd, n):
    """a with a a at the bounds of fe_sqr: limbs at sqrt(limit) (the doubled limb the products take is ~2^30.7), |a|^2 at 2^261 m"""
    T = RADIX * m
    out = []
    while len(out) < n:
        kind = len(out) % 3
        f = rnd.uniform(0.99, 0.9999)
        L = int((f * MUL_LIMB_LIMIT) ** 0.5)
        if kind == 0:
            a = _signed_limbs(rnd, L, rnd.randrange(-(1 << 20), 1 << 20))
        elif kind == 1:
            A = int((f * T) ** 0.5)
            a = limbs(A if rnd.randrange(2) else -A)
        else:
            A = int((f * T) ** 0.5)
            a = _with_value(rnd, L, A if rnd.randrange(2) else -A)
        if legal_mul(a, a, m):
            out.append(a)
    return out


def saturating_mulsub(m, rnd, n):
    """(a, b, c, d) at fe_mulsub's bounds: max|a||b| + max|c||d| in [0.99, 1) of its column limit, |a b| + |c d| in [0.99, 1) of
    2^261 m, and both"""
    T = RADIX * m
    out = []
    while len(out) < n:
        kind = len(out) % 3
        f = rnd.uniform(0.99, 0.9995)
        share = rnd.choice((0.5, rnd.uniform(0.05, 0.95), 0.999))
        S1, S2 = f * MULSUB_LIMB_LIMIT * share, f * MULSUB_LIMB_LIMIT * (1 - share)
        if kind == 0:
            La = int(rnd.uniform(max(2 ** 27.5, S1 / 2 ** 30.9), 2 ** 30.5)); Lc = int(rnd.uniform(max(2 ** 27.5, S2 / 2 ** 30.9), 2 ** 30.5))
            ops = [_signed_limbs(rnd, La, rnd.randrange(-(1 << 20), 1 << 20)), _signed_limbs(rnd, max(1, int(S1 / La)), rnd.randrange(-(1 << 20), 1 << 20)),
                   _signed_limbs(rnd, Lc, rnd.randrange(-(1 << 20), 1 << 20)), _signed_limbs(rnd, max(1, int(S2 / Lc)), rnd.randrange(-(1 << 20), 1 << 20))]
        elif kind == 1:
            V1, V2 = int(f * T * share), int(f * T * (1 - share))
            A = int(2 ** rnd.uniform(255, 259.5)) + rnd.getrandbits(230); C = int(2 ** rnd.uniform(255, 259.5)) + rnd.getrandbits(230)
            ops = [limbs(A), limbs(-(V1 // A) if rnd.randrange(2) else V1 // A), limbs(-C if rnd.randrange(2) else C), limbs(max(1, V2 // C))]
        else:
            L1, L2 = int(S1 ** 0.5), int(max(S2, 1) ** 0.5)
            V1, V2 = int(f * T * share), int(f * T * (1 - share))
            a = _with_value(rnd, L1, int(V1 ** 0.5) or 1)
            b = _with_value(rnd, L1, -(V1 // abs(value(a) or 1)))
            c = _with_value(rnd, L2, int(V2 ** 0.5) or 1)
            d = _with_value(rnd, L2, V2 // abs(value(c) or 1))
            ops = [a, b, c, d]
        if legal_mulsub(*ops, m):
            out.append(tuple(ops))
    return out


def random_legal_rows(np_rng, n, kind):
    """n random operand rows legal for every product (vectorised): limbs 0..7 within +-2^b for a per-row b <= 29 (or normalised
    canonical-range values), top limbs within +-2^22: max|a_j| max|b_j| <= 2^58, |a b| < 2^508.1 < 2^261 m."""
    rows = np.zeros((n, 4 * NL), dtype=np.int64)
    for s in range(4):
        bits = np_rng.integers(1, 30, size=(n, 1))
        span = (np.int64(1) << bits) - 1
        if kind == "signed":
            low = np_rng.integers(-(1 << 29) + 1, 1 << 29, size=(n, NL - 1)) % (2 * span + 1) - span
            top = np_rng.integers(-(1 << 22), (1 << 22) + 1, size=n)
        else:                                          # normalised values in [0, 2^254)
            low = np_rng.integers(0, 1 << 29, size=(n, NL - 1))
            top = np_rng.integers(0, 1 << 22, size=n)
        rows[:, NL * s:NL * s + NL - 1] = low
        rows[:, NL * s + NL - 1] = top
    return rows.astype(np.int32)


def place(random_rows, edge_rows, seed):
    """Copies of every edge row at lanes 0, 31, 32 and 63 of two waves each, the waves spread over the whole launch; the other rows
    stay random.  Returns the array and the indices that hold edges."""
    arr = random_rows.copy()
    n = arr.shape[0]
    waves = n // 64
    assert 2 * len(edge_rows) <= waves // 2, "too few rows for the edge copies"
    rnd = random.Random(seed)
    used = set()
    idx = []
    for e, r in enumerate(edge_rows):
        for t in range(2):
            for lane in (0, 31, 32, 63):
                w = rnd.randrange(waves)
                while (w, lane) in used:
                    w = (w + 1) % waves
                used.add((w, lane))
                arr[w * 64 + lane] = r
                idx.append(w * 64 + lane)
    return arr, np.array(sorted(idx), dtype=np.int64)


# ----- expected results by big-integer arithmetic ---------------------------------------------------------------------------------
def check_values(op, which, inp, out, idx):
    """For the rows idx of one op's operands and results: the value the header defines (a b 2^-261 mod m, ...) and the output range it
    states.  Returns a list of failure descriptions (empty = pass)."""
    m = MODS[which]
    rinv = pow(RADIX, -1, m)
    bad = []
    sub_in = np.asarray(inp)[idx]
    sub_out = np.asarray(out)[idx]
    va, vb, vc, vd = (values(sub_in, s) for s in range(4))
    vr, vs = values(sub_out, 0), values(sub_out, 1)
    for i in range(len(idx)):
        a, b, c, d, r, s = va[i], vb[i], vc[i], vd[i], vr[i], vs[i]
        rl, sl = sub_out[i, :NL], sub_out[i, NL:]
        good = True
        if op in (MUL, MUL_ILP, SQR, MUL2, SQR2, MULSUB):
            if op == MULSUB:
                want = [((a * b - c * d) * rinv) % m]
            elif op in (MUL, MUL_ILP):
                want = [(a * b * rinv) % m]
            elif op == SQR:
                want = [(a * a * rinv) % m]
            elif op == MUL2:
                want = [(a * b * rinv) % m, (c * d * rinv) % m]
            else:
                want = [(a * a * rinv) % m, (c * c * rinv) % m]
            for w, v, l in zip(want, (r, s), (rl, sl)):
                good &= v % m == w and -m < v < 2 * m and normalised(l)
        elif op in (ADD, SUB, DBL):
            other = b if op == ADD else (-b if op == SUB else a)
            la, lb = sub_in[i, :NL].astype(np.int64), sub_in[i, NL:2 * NL].astype(np.int64)
            wl = la + (lb if op == ADD else (-lb if op == SUB else la))
            good = r == a + other and np.array_equal(rl.astype(np.int64), wl)
        elif op == NORM:
            good = r == a and normalised(rl)
        elif op == CANON:
            good = r == a % m and normalised(rl)
        elif op == IS_ZERO_MOD:
            good = int(rl[0]) == (1 if a % m == 0 else 0)
        elif op == REDUCE:
            good = r % m == a % m and -m < r < 2 * m and normalised(rl)
        elif op == REDUCE_SMALL:
            good = r % m == a % m and -m < 10000 * r < 10001 * m and normalised(rl)     # (-0.0001 m, 1.0001 m), field29.h
        elif op == FROM_WIRE:
            w = words_value(sub_in[i])
            good = r % m == (w << 5) % m and -m < r < 2 * m and normalised(rl)
        elif op == TO_WIRE:
            got = words_value(rl)
            good = got == (a * pow(32, -1, m)) % m
        elif op == WIRE_TO_CANONICAL:
            got = words_value(rl)
            good = got == (words_value(sub_in[i]) * pow(1 << 256, -1, m)) % m
        elif op == INVERT:
            want = 0 if a % m == 0 else (RADIX * RADIX * pow(a, -1, m)) % m
            good = r % m == want and -m < r < 2 * m and normalised(rl)
        if not good:
            bad.append((int(idx[i]), NAMES[op], which, list(map(int, sub_in[i])), list(map(int, sub_out[i]))))
            if len(bad) >= 5:
                break
    return bad


# ----- one operand set per primitive ----------------------------------------------------------------------------------------------
def edge_rows(op, which, seed=0):
    """the deterministic edge operands of one primitive (rows of 36 ints), every one legal for it"""
    m = MODS[which]
    rnd = random.Random(1000 * op + 10 * which + seed)
    edges = canonical_edges(m)
    lazy = lazy_values(m, rnd, 40)
    pats = extreme_patterns(rnd)
    rows = []
    if op in (MUL, MUL_ILP, MUL2, MULSUB):
        pairs = [(p, q) for p in pats for q in pats[:12]]
        pairs += [(limbs(x), limbs(y)) for x in edges for y in edges if legal_mul(limbs(x), limbs(y), m)]
        pairs += [(unnormalise(limbs(x), rnd), unnormalise(limbs(y), rnd)) for x, y in zip(lazy, reversed(lazy))]
        pairs = [p for p in pairs if legal_mul(p[0], p[1], m)]
        pairs += saturating_mul_pairs(m, rnd, 600)
        if op == MULSUB:
            quads = saturating_mulsub(m, rnd, 900)
            quads += [(a, b, c, d) for (a, b), (c, d) in zip(pairs, pairs[7:] + pairs[:7]) if legal_mulsub(a, b, c, d, m)]
            rows = [row(*q) for q in quads]
        elif op == MUL2:
            rows = [row(a, b, c, d) for (a, b), (c, d) in zip(pairs, pairs[5:] + pairs[:5])]
        else:
            rows = [row(a, b) for a, b in pairs]
    elif op in (SQR, SQR2):
        sq = [p for p in pats if legal_mul(p, p, m)] + [limbs(x) for x in edges if legal_mul(limbs(x), limbs(x), m)]
        sq += [unnormalise(limbs(x), rnd) for x in lazy]
        sq += saturating_squares(m, rnd, 600)
        rows = [row(a, [0] * NL, sq[(k * 7 + 3) % len(sq)]) for k, a in enumerate(sq)]
    elif op in (ADD, SUB, DBL):
        big = (1 << 31) - 1
        cases = [([big // 2] * 9, [big - big // 2] * 9), ([-(1 << 30)] * 9, [-(1 << 30)] * 9), ([big] * 9, [0] * 9), ([-(1 << 31)] * 9, [0] * 9),
                 ([(1 << 30) - 1] * 9, [(1 << 30)] * 9), ([-(1 << 30)] * 9, [(1 << 30) - 1] * 9)]
        cases += [(p, q) for p in pats for q in pats[:6]]
        cases += [(limbs(x), limbs(y)) for x, y in zip(lazy, reversed(lazy))]

        def ok(a, b):
            if op == DBL:
                b = a
            sg = -1 if op == SUB else 1
            return all(-(1 << 31) <= x + sg * y < (1 << 31) for x, y in zip(a, b))
        rows = [row(a, b) for a, b in cases if ok(a, b)]
    elif op == NORM:
        vs = [unnormalise(limbs(x), rnd) for x in lazy + edges] + pats
        vs += [[(1 << 31) - 5] * 8 + [0], [-(1 << 31) + 4] * 8 + [0], [(1 << 31) - 1] + [0] * 8]
        rows = [row(a) for a in vs]
    elif op in (CANON, IS_ZERO_MOD, INVERT):
        vs = [x for x in edges + lazy if -m < x < 2 * m]
        rows = [row(limbs(x)) for x in vs]
    elif op in (REDUCE, REDUCE_SMALL):
        lim = REDUCE_LIMIT * m          # the C predicates compare in double: edges stay 1e-9 inside
        vs = [x for x in edges + lazy if abs(x) < lim] + [lim - lim // 10 ** 9, -(lim - lim // 10 ** 9), lim - m, 128 * m - 1, -(128 * m - 1)]
        vs += [rnd.randrange(-lim + 1, lim) for _ in range(200)]
        rows = [row(limbs(x)) for x in vs] + [row(unnormalise(limbs(x), rnd)) for x in vs[:200]]
        rows = [r_ for r_ in rows if abs(value(r_[:NL])) < lim]
    elif op in (FROM_WIRE, WIRE_TO_CANONICAL):
        vs = [x for x in edges if 0 <= x < m] + [rnd.randrange(m) for _ in range(200)]
        rows = [row(value_words(x)) for x in vs]
    elif op == TO_WIRE:
        lim = REDUCE_LIMIT * m
        vs = [x for x in edges + lazy if abs(x) < lim] + [lim - lim // 10 ** 9, -(lim - lim // 10 ** 9)] + [rnd.randrange(-lim + 1, lim) for _ in range(200)]
        rows = [row(limbs(x)) for x in vs]
    return to_array(rows)


def random_rows(op, which, n, seed=0):
    """n random legal operand rows of one primitive"""
    m = MODS[which]
    np_rng = np.random.default_rng(7919 * op + 31 * which + seed)
    if op in PRODUCTS or op in (ADD, SUB, DBL, NORM):
        half = n // 2
        return np.concatenate([random_legal_rows(np_rng, half, "signed"), random_legal_rows(np_rng, n - half, "normalised")])
    rnd = random.Random(104729 * op + which + seed)
    if op in (CANON, IS_ZERO_MOD, INVERT):
        vs = [rnd.randrange(-m + 1, 2 * m) for _ in range(n)]
    elif op in (REDUCE, REDUCE_SMALL, TO_WIRE):
        vs = [rnd.randrange(-REDUCE_LIMIT * m + 1, REDUCE_LIMIT * m) for _ in range(n)]
    else:
        return to_array([row(value_words(rnd.randrange(m))) for _ in range(n)])
    return to_array([row(limbs(x)) for x in vs])


# ----- point formulas and NAF recoding (tests/devcheck/dc_prims.h dc_curve / dc_naf) ----------------------------------------------
MADD, PADD, PDBL = range(3)
CURVE_NAMES = ["xyzz_madd", "xyzz_add", "xyzz_dbl"]


def curve_cases(points, rnd, n_random=200):
    """(P1, P2, sign) triples: random pairs plus the exceptional cases of every formula -- the same point, the negated point, the
    identity (P1 = None), and for xyzz_add the opposite stored points (P1 = -3 P2)"""
    import pyref
    cases = []
    for _ in range(n_random):
        cases.append((points[rnd.randrange(len(points))], points[rnd.randrange(len(points))], rnd.randrange(2)))
    for k in range(24):
        q = points[rnd.randrange(len(points))]
        cases += [(q, q, 0), (q, q, 1), (pyref.ec_neg(q), q, 0), (pyref.ec_neg(q), q, 1), (None, q, 0), (None, q, 1),
                  (pyref.ec_mul(R_ - 3, q), q, 0), (pyref.ec_mul(2, q), q, 1)]
    return cases


def curve_expected(op, p1, p2, sign):
    import pyref
    if op == MADD:
        return pyref.ec_add(p1, pyref.ec_neg(p2) if sign else p2)
    s = pyref.ec_add(p1, p2)
    if op == PADD:
        return pyref.ec_add(s, pyref.ec_mul(2, p2))
    return pyref.ec_mul(2, s)


def curve_rows(cases):
    import pyref
    rows = np.zeros((len(cases), 33), np.uint32)
    for i, (p1, p2, sign) in enumerate(cases):
        rows[i, :16] = pyref.point_to_wire(p1).view(np.uint32)
        rows[i, 16:32] = pyref.point_to_wire(p2).view(np.uint32)
        rows[i, 32] = sign
    return rows


def xyzz_wire_to_affine(out32):
    """X, Y, ZZ, ZZZ wire words -> affine ints (None = identity); asserts ZZ^3 == ZZZ^2"""
    import pyref
    w = np.ascontiguousarray(out32, dtype=np.uint32).view(np.uint64).reshape(4, 4)
    X, Y, ZZ, ZZZ = (pyref.fq_from_mont(w[i]) for i in range(4))
    if ZZ == 0:
        return None
    assert pow(ZZ, 3, P) == pow(ZZZ, 2, P)
    return (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)


NAF_WIDTHS = (10, 14, 16, 17, 18)


def naf_rows(rnd, n_random=600):
    special = [0, 1, 2, 3, R_ - 1, R_ - 2, 1 << 253, (1 << 254) - 1, (1 << 254) - (1 << 200), 0xFFFFFFFF, 1 << 32, (1 << 64) - 1,
               int("01" * 127, 2), int("10" * 127, 2), int("0111" * 63, 2), (1 << 253) + (1 << 17) - 1, (1 << 248) - 1]
    ks = special + [rnd.randrange(R_) for _ in range(n_random)] + [rnd.randrange(1 << rnd.randrange(1, 254)) for _ in range(n_random // 3)]
    scal = np.array([[(k >> (32 * j)) & 0xFFFFFFFF for j in range(8)] for k in ks for _ in NAF_WIDTHS], np.uint32)
    width = np.array([w for _ in ks for w in NAF_WIDTHS], np.int32)
    return ks, scal, width


def naf_value(out_row, w):
    """the scalar the digits of one dc_naf row encode; asserts the digit invariants (odd, < 2^(w-1), >= w apart, position <= 254)"""
    n = int(out_row[0])
    assert 0 <= n <= min(63, 254 // w + 1)
    val, last = 0, None
    for t in range(n):
        d = int(out_row[1 + t])
        neg, pos, key = d >> 31, (d >> 20) & 0x7FF, d & 0xFFFFF
        mag = 2 * key + 1
        assert mag < (1 << (w - 1)) and pos <= 254 and (last is None or pos >= last + w)
        last = pos
        val += (-mag if neg else mag) << pos
    return val
