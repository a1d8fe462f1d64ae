"""-m gpu: the located coset verifiers with their pairing checks on the device (`kzg_ctx_set_locate_pairings(ctx, 1)`).

Mode 1 keeps the root check on the host and, after a failing root over more than one group, evaluates EVERY group's own equation as one
batch on the device (csrc/pairing.hip) in place of the host's binary search.  Truth is mode 0 on the same inputs: statuses, rows, flags,
counts and group maps are equal.  The worlds and plants are those of tests/test_gpu_retrieve_tolerant.py (shapes `tiny` and `wave`).

The documented count of checks (include/kzg_bn254_mi355x.h, "pairing checks of a located batch"), per located pass over S non-empty groups:
    1                 the root holds, or S = 1 (a failing root over one group names it)
    1 + S             otherwise
and for the tolerant retriever 1 (the batch equation) + on a reject the pass over the blobs + the pass over the decodable items of the
bad blobs, when there are any."""
import random

import numpy as np
import pytest

import test_gpu_retrieve_tolerant as T
from test_gpu_retrieve_tolerant import EQUATION, GOOD, PLANTS, plant, tolerant, world_of

pytestmark = pytest.mark.gpu
NAMES = ["tiny", "wave"]


@pytest.fixture(scope="module")
def k():
    import rust_kzg_bn254_amd as k
    k.load()
    k.default_context()
    return k


@pytest.fixture()
def device_pairings(k):
    """run(f): f() in mode 0, then in mode 1; the finalizer puts the context back to mode 0 whatever happened"""
    ctx = k.default_context()

    def run(f):
        ctx.set_locate_pairings(0)
        a = f()
        ctx.set_locate_pairings(1)
        try:
            b = f()
        finally:
            ctx.set_locate_pairings(0)
        return a, b

    yield run
    ctx.set_locate_pairings(0)


def pass_checks(groups):
    return 1 if groups <= 1 else 1 + groups


def retrieve_checks(w, status):
    """the documented count for the tolerant retriever in mode 1"""
    if not (status == EQUATION).any():
        return 1
    bad_blobs = [b for b in range(w.B) if (status[b * w.count:(b + 1) * w.count] == EQUATION).any()]
    items = sum(int((status[b * w.count:(b + 1) * w.count] == GOOD).sum() + (status[b * w.count:(b + 1) * w.count] == EQUATION).sum()) for b in bad_blobs)
    return 1 + pass_checks(w.B) + (pass_checks(items) if items else 0)


def same_result(a, b):
    """everything `tolerant` returns but the count of checks"""
    assert a[0] == 0 and b[0] == 0
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:5] == b[3:5]      # item and blob statuses, bad items, unrecovered
    assert a[6] == b[6] and np.array_equal(a[7], b[7])                                          # rows, flags
    assert np.array_equal(a[10], b[10])                                                         # the weights used


@pytest.mark.parametrize("name", NAMES)
def test_tolerant_retrieval_equals_the_host_search(k, device_pairings, name):
    w = world_of(k, name)
    ys_be, pf_be, status = plant(w, PLANTS[name])
    weights = k.verifier.compute_multiproof_r_powers_bytes(w.commitments_be, w.ci, w.ki, ys_be, pf_be, w.n, w.l)
    for rp in (None, weights):                                                                  # derived and supplied transcript weights
        host, dev = device_pairings(lambda: tolerant(k, w, ys_be, pf_be, bound=w.d, form=0, out_len=w.d, r_powers=rp))
        same_result(host, dev)
        assert np.array_equal(dev[1], status)
        T.check_bound(w, status, host[5])
        print(name, "checks: host search", host[5], "device leaves", dev[5])
        assert dev[5] == retrieve_checks(w, status), (dev[5], retrieve_checks(w, status))
    # evaluation rows through the Python surface
    a, b = device_pairings(lambda: k.verifier.retrieve_blobs_bytes_tolerant(w.commitments_be, w.rows, ys_be, pf_be, w.n, w.l, w.srs, use_count=w.use, g2_tau_l=w.g2))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("name", NAMES)
def test_a_good_batch_spends_one_check_in_both_modes(k, device_pairings, name):
    w = world_of(k, name)
    host, dev = device_pairings(lambda: tolerant(k, w, w.ys_be, w.pf_be, bound=w.d, out_len=w.d))
    same_result(host, dev)
    assert host[5] == 1 and dev[5] == 1 and not dev[1].any() and dev[6] == b"".join(w.original)
    for groups in ("commitment", "item"):
        a, b = device_pairings(lambda: k.verifier.locate_bad_multiproofs_bytes(w.commitments_be, w.ci, w.ki, w.ys_be, w.pf_be, w.n, w.l, w.srs, w.g2, groups=groups))
        assert a[0].all() and b[0].all() and a[1] == 1 and b[1] == 1


@pytest.mark.parametrize("name", NAMES)
def test_group_maps_equal_the_host_search(k, device_pairings, name):
    w = world_of(k, name)
    v = k.verifier
    plants = [(i, kind) for i, kind in PLANTS[name] if kind in ("flip", "swap", "moved")]       # what decodes
    ys_be, pf_be, status = plant(w, plants)
    ys, pf = v.decode_coset_items(ys_be, pf_be, w.l)
    rnd = random.Random(name)
    partition = [rnd.randrange(7) for _ in range(w.N)]                                          # 9 groups, two of them empty
    weights = v.compute_multiproof_r_powers(w.commitments, w.ci, w.ki, ys, pf, w.n)
    for groups, n_groups, non_empty in (("commitment", None, w.B), ("item", None, w.N), (partition, 9, len(set(partition))), ([0] * w.N, 1, 1)):
        for rp in (None, weights):
            (want, host_checks), (good, checks) = device_pairings(
                lambda: v.locate_bad_multiproofs(w.commitments, w.ci, w.ki, ys, pf, w.n, w.srs, w.g2, r_powers=rp, groups=groups, n_groups=n_groups))
            what = groups if isinstance(groups, str) else "array of %d" % n_groups
            assert np.array_equal(good, want), what
            assert not good.all() and checks == pass_checks(non_empty), (what, checks)
            assert host_checks <= T.max_checks(non_empty, int((~want).sum())), what
        (want, _), (good, checks) = device_pairings(
            lambda: v.locate_bad_multiproofs_bytes(w.commitments_be, w.ci, w.ki, ys_be, pf_be, w.n, w.l, w.srs, w.g2, groups=groups, n_groups=n_groups))
        assert np.array_equal(good, want) and checks == pass_checks(non_empty)
        if groups == "item":
            assert np.array_equal(~good, status == EQUATION)
        if groups == "commitment":
            assert (~good).tolist() == [bool((status[b * w.count:(b + 1) * w.count] == EQUATION).any()) for b in range(w.B)]


def test_the_mode_is_per_context_and_checked(k):
    ctx = k.default_context()
    for bad in (-1, 2, 7):
        with pytest.raises(ValueError):
            ctx.set_locate_pairings(bad)
    other = k._lib.Context(0)
    try:
        other.set_locate_pairings(1)                                                             # another context's mode is its own
        w = world_of(k, "tiny")
        good, checks = k.verifier.locate_bad_multiproofs_bytes(w.commitments_be, w.ci, w.ki, *plant(w, [(0, "flip")])[:2], w.n, w.l, w.srs, w.g2, groups="item")
        assert (~good).tolist() == [True] + [False] * (w.N - 1)
        assert 1 < checks <= T.max_checks(w.N, 1) < 1 + w.N                                      # the default context still searches on the host: not 1 + N leaves
    finally:
        other.close()
