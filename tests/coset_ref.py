"""Big-integer restatement of the verification of coset proofs (`kzg_coset_interpolate_rlc`, `kzg_verify_multiproof_batch`): shared by
tests/test_multiproof_verify_host.py and tests/test_gpu_multiproof_verify.py.  Everything is over Fr with python ints."""
from pyref import R_, root_of_unity


def ifft(vals):
    """IFFT_l over the library's l-th root, natural order in and out, 1 / l included (O(l log l); pyref.dft(.., inverse=True) is the
    O(l^2) definition it is checked against)."""
    l = len(vals)
    winv = pow(root_of_unity(l.bit_length() - 1), -1, R_)

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

    linv = pow(l, -1, R_)
    return [x * linv % R_ for x in rec(list(vals), winv)]


def interpolation_coeffs(ys, k, n):
    """Coefficients a_t = w^(-k t) IFFT_l(ys)_t of the polynomial of degree < l with I(w^k w_l^j) = ys[j], w the n-th root."""
    winv_k = pow(root_of_unity(n.bit_length() - 1), -k, R_)
    out, cur = [], 1
    for a in ifft(ys):
        out.append(a * cur % R_)
        cur = cur * winv_k % R_
    return out


def coset_rlc(ys_list, ks, weights, n):
    """A_t = sum_i weights[i] w^(-ks[i] t) IFFT_l(ys_list[i])_t"""
    l = len(ys_list[0])
    acc = [0] * l
    for ys, k, r in zip(ys_list, ks, weights):
        for t, a in enumerate(interpolation_coeffs(ys, k, n)):
            acc[t] = (acc[t] + r * a) % R_
    return acc


def batch_equation_holds(tau, n, l, commitments, rows, ks, ys_list, proofs, weights):
    """The batch equation with every group element replaced by its discrete logarithm (commitments = f(tau), proofs = q_k(tau)) and the
    pairing with [tau^l]_2 by a product with tau^l."""
    w = root_of_unity(n.bit_length() - 1)
    A = coset_rlc(ys_list, ks, weights, n)
    lhs = sum(r * p for r, p in zip(weights, proofs)) % R_ * pow(tau, l, R_) % R_
    rhs = sum(r * commitments[c] for r, c in zip(weights, rows))
    rhs -= sum(a * pow(tau, t, R_) for t, a in enumerate(A))
    rhs += sum(r * pow(w, k * l, R_) * p for r, k, p in zip(weights, ks, proofs))
    return lhs == rhs % R_
