"""Big-integer restatement of erasure decoding (`kzg_recover_from_cosets`): shared by tests/test_recover_math_host.py and
tests/test_gpu_recover.py.  Everything is over Fr with python ints.  `fft` is O(n log n) and serves any size; `recover` takes its
vanishing values as naive products and is meant for n <= 64 (the first test file also runs it at 2 048 once)."""
from pyref import R_, root_of_unity

G = 5                                                   # the shift of the second domain {G w^i}: the library's multiplicative generator


def fft(vals, inverse=False):
    """ark-poly's fft / ifft on the domain {w^i}, w the library's n-th root: natural order in and out, 1 / n included in the inverse."""
    n = len(vals)
    w = root_of_unity(n.bit_length() - 1)
    if inverse:
        w = pow(w, -1, R_)

    def rec(v, w):
        if len(v) == 1:
            return v
        ev, od = rec(v[0::2], w * w % R_), rec(v[1::2], w * w % R_)
        h = len(v) // 2
        out, cur = [0] * len(v), 1
        for t in range(h):
            x = od[t] * cur % R_
            out[t] = (ev[t] + x) % R_
            out[t + h] = (ev[t] - x) % R_
            cur = cur * w % R_
        return out

    out = rec(list(vals), w)
    if inverse:
        ninv = pow(n, -1, R_)
        out = [x * ninv % R_ for x in out]
    return out


def coset_rows(evals, l, ks):
    """Rows ks of KZG.cosets: row k = evals[k::m], the values on {w^(k + j m) : j < l}."""
    m = len(evals) // l
    return [[evals[k + j * m] for j in range(l)] for k in ks]


def recover(n, l, ks, ys, degree_bound=None):
    """(coefficients, consistent) of the polynomial of degree < len(ks) l through the values ys[i] of the cosets ks[i] of the n-point
    domain: the steps of recover.hip, one line each."""
    m = n // l
    wm = pow(root_of_unity(n.bit_length() - 1), l, R_)                          # the m-th root w^l
    present = set(ks)
    assert len(present) == len(ks) and all(0 <= k < m for k in ks)
    missing = [k for k in range(m) if k not in present]

    roots = [1] * m
    for i in range(1, m):
        roots[i] = roots[i - 1] * wm % R_

    def z_at(y):
        acc = 1
        for k in missing:
            acc = acc * (y - roots[k]) % R_
        return acc

    s = pow(G, l, R_)
    zd = [z_at(roots[i]) for i in range(m)]                                     # 1. z on the m-th roots ...
    zs = [z_at(s * roots[i] % R_) for i in range(m)]                            #    ... and on the shifted ones
    D = [0] * n
    for k, row in zip(ks, ys):                                                  # 2. values times Z, zero on the missing cosets
        for j in range(l):
            D[k + j * m] = row[j] * zd[k] % R_
    P = fft(D, inverse=True)                                                    # 3. f Z
    Pe = fft([c * pow(G, t, R_) % R_ for t, c in enumerate(P)])                 # 4. (f Z)(G w^i)
    Q = [Pe[i] * pow(zs[i % m], -1, R_) % R_ for i in range(n)]                 # 5. f(G w^i)
    ginv = pow(G, -1, R_)
    f = [c * pow(ginv, t, R_) % R_ for t, c in enumerate(fft(Q, inverse=True))]   # 6. the coefficients
    bound = len(ks) * l if not degree_bound else degree_bound
    return f, not any(f[bound:])                                                # 7.
