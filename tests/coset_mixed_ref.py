"""Big-integer restatement of the verification of coset proofs of MIXED shapes (`kzg_coset_interpolate_rlc_mixed`,
`kzg_compute_multiproof_r_powers_mixed`, `kzg_verify_multiproof_batch_mixed`), built on coset_ref: shared by
tests/test_multiproof_verify_mixed_host.py and tests/test_gpu_multiproof_verify_mixed.py.  A class is a pair (n, l); item i has the class
classes[class_indices[i]].  Everything is over Fr with python ints."""
import hashlib

import coset_ref
from pyref import R_, root_of_unity


def mixed_rlc(classes, class_indices, ks, ys_list, weights):
    """A_t = sum_{i : l_i > t} weights[i] w_i^(-ks[i] t) IFFT_{l_i}(ys_list[i])_t for t < l_max, l_max over ALL classes"""
    acc = [0] * max(l for _, l in classes)
    for s, k, ys, r in zip(class_indices, ks, ys_list, weights):
        n, l = classes[s]
        assert len(ys) == l
        for t, a in enumerate(coset_ref.interpolation_coeffs(ys, k, n)):
            acc[t] = (acc[t] + r * a) % R_
    return acc


def mixed_equation_holds(tau, classes, class_indices, commitments, rows, ks, ys_list, proofs, weights, tau_powers=None):
    """The mixed equation with every group element replaced by its discrete logarithm (commitments = f(tau), proofs = q_k(tau)) and the
    pairing with the G2 point of class s by a product with its discrete logarithm tau_powers[s] (default tau^(l_s)): one term per DISTINCT
    chunk length, taken from the first class of that length as the library takes it."""
    if tau_powers is None:
        tau_powers = [pow(tau, l, R_) for _, l in classes]
    A = mixed_rlc(classes, class_indices, ks, ys_list, weights)
    first_of_len = {}
    for s, (_, l) in enumerate(classes):
        first_of_len.setdefault(l, s)
    L = {}
    for s, r, p in zip(class_indices, weights, proofs):
        l = classes[s][1]
        L[l] = (L.get(l, 0) + r * p) % R_
    lhs = sum(v * tau_powers[first_of_len[l]] for l, v in L.items()) % R_
    rhs = sum(r * commitments[c] for r, c in zip(weights, rows))
    rhs -= sum(a * pow(tau, t, R_) for t, a in enumerate(A))
    for s, r, k, p in zip(class_indices, weights, ks, proofs):
        n, l = classes[s]
        rhs += r * pow(root_of_unity(n.bit_length() - 1), k * l, R_) * p
    return lhs == rhs % R_


def compressed(pt):
    """ark-compressed G1: pt is None (identity) or (x, y) as ints"""
    from pyref import P
    if pt is None:
        return bytes(31) + b"\x40"
    b = bytearray(pt[0].to_bytes(32, "little"))
    if pt[1] > (P - 1) // 2:
        b[31] |= 0x80
    return bytes(b)


def mixed_r(classes, class_indices, commitments, rows, ks, ys_list, proofs):
    """r of the mixed transcript with hashlib; commitments / proofs as points (None or (x, y)), values as ints"""
    data = b"KZGBN254_COSETMIXED__V1_" + len(classes).to_bytes(8, "big")
    for n, l in classes:
        data += n.to_bytes(8, "big") + l.to_bytes(8, "big")
    data += len(commitments).to_bytes(8, "big") + len(class_indices).to_bytes(8, "big")
    data += b"".join(s.to_bytes(8, "big") for s in class_indices)
    data += b"".join(compressed(c) for c in commitments)
    for s, c, k, ys, p in zip(class_indices, rows, ks, ys_list, proofs):
        assert len(ys) == classes[s][1]
        item = b"KZGBN254_COSETITEM___V1_" + c.to_bytes(8, "big") + k.to_bytes(8, "big")
        item += b"".join(v.to_bytes(32, "big") for v in ys) + compressed(p)
        data += hashlib.sha256(item).digest()
    return int.from_bytes(hashlib.sha256(data).digest(), "big") % R_
