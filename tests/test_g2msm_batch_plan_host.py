"""CPU: the groups of the G2 MSM planner (csrc/g2msm_plan.h: g2_batch_group, g2_make_plan, g2_plan_status) as a plain g++
program, no GPU and no library (tests/hostcheck/g2msm_plan_grid.h states the invariants: the three caps of a group hold and one
more blob breaks one of them or meets the caller's cap; every buffer is as large as the kernels index it; seg * nl covers the entries; at
most four lanes per bucket; batched = 0 exactly when the rule says so) -- and `kzg_msm_g2_batch_info`, the pure query of the built library,
which must agree with that program and return the documented errors."""
import ctypes as C
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg-bn254_amd", "csrc")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("g2b") / "g2msm_plancheck")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, os.path.join(HERE, "hostcheck", "g2msm_plancheck.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = []
    for ln in r.stdout.splitlines():
        if " count=" not in ln: continue                               # (the lines of one blob: tests/test_g2msm_plan_host.py)
        rows.append({k: int(v) for k, v in (f.split("=") for f in ln.split())})
    return rows


def test_every_plan_of_the_grid_keeps_its_invariants_and_the_grid_covers_every_path(plans):
    ns = {r["n"] for r in plans}
    for k in range(21):
        for n in (2 ** k - 1, 2 ** k, 2 ** k + 1):
            assert n in ns or n == 0 or n > 2 ** 20, n
    assert {r["nb"] for r in plans} == {1, 2} and {r["count"] for r in plans} == {1, 2, 3, 5, 16, 64, 95, 96, 1024} and {r["max"] for r in plans} == {0, 1, 2}
    batched = [r for r in plans if r["batched"]]
    # both sort forms and both scan forms
    for field in ("small", "scan1"):
        assert {r[field] for r in batched} == {0, 1}, field
    # the result cap binds: n = 4 096, two base sets -> 95 blobs of the 96 or 1 024 asked for
    for count in (96, 1024):
        r, = [r for r in batched if (r["n"], r["nb"], r["count"], r["max"]) == (4096, 2, count, 0)]
        assert r["group"] == 95 and r["result_binds"] and not r["entry_binds"] and r["c"] == 6 and r["W"] == 43
    r, = [r for r in batched if (r["n"], r["nb"], r["count"], r["max"]) == (4096, 2, 95, 0)]
    assert r["group"] == 95
    # the entry cap binds: 19 windows of 2^20 scalars -> 6 blobs
    r, = [r for r in batched if (r["n"], r["nb"], r["count"], r["max"]) == (1 << 20, 1, 16, 0)]
    assert r["group"] == 6 and r["entry_binds"] and not r["result_binds"] and r["scan1"] == 0
    assert any(r["entry_binds"] and not r["result_binds"] for r in batched) and any(r["result_binds"] and not r["entry_binds"] for r in batched)
    # the caller's cap
    assert all(r["group"] <= 2 for r in batched if r["max"] == 2) and any(r["group"] == 2 for r in batched if r["max"] == 2)
    assert all(r["group"] == 1 for r in batched if r["max"] == 1)
    # every shape of the grid batches (a blob of at most 2^20 scalars leaves room for two), the lane cap is met somewhere and slack somewhere
    assert len(batched) == len(plans)
    assert any(r["nl"] == max(256, (4 * r["G"] + 255) // 256 * 256) and r["seg"] > 4 for r in batched)
    assert any(r["nl"] < (4 * r["G"] + 255) // 256 * 256 for r in batched)
    # launches: the sort's and six, whatever nb
    for r in batched:
        assert r["launches"] == 2 + r["small"] + 1 + (1 if r["scan1"] else 3) + 1 + 6


def test_the_planner_header_includes_no_hip():
    src = open(os.path.join(CSRC, "g2msm_plan.h")).read()
    assert not any("hip" in ln for ln in src.splitlines() if ln.startswith("#include"))


def test_info_agrees_with_the_planner_and_returns_the_documented_errors(plans):
    import rust_kzg_bn254_amd as k
    L = k._lib
    lib = L.load()                                                     # loading needs no GPU
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "kzg_bn254_mi355x.h")).read(), flags=re.S)
    m = re.search(r"typedef struct kzg_g2_batch_info \{(.*?)\}", header, flags=re.S)
    fields = [f.strip() for ln in m.group(1).splitlines() if ln.strip() for f in ln.split(";")[0].split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in L.G2BatchInfo._fields_], fields
    assert C.sizeof(L.G2BatchInfo) == 4 * 8 + 10 * 4
    for name, n_args in (("kzg_msm_g2_srs_batch", 8), ("kzg_msm_g2_srs_batch_device", 8), ("kzg_commit_with_length_proof_batch", 13),
                         ("kzg_ctx_set_g2_batch_group", 2), ("kzg_msm_g2_batch_info", 5)):
        assert hasattr(lib, name) and len(L.PROTOTYPES[name][1]) == n_args, name
        decl = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert decl and len(decl.group(1).split(",")) == n_args, name
    info = k.helpers.g2_batch_info
    by_key = {(r["n"], r["nb"], r["count"], r["max"]): r for r in plans}
    for key in ((4096, 2, 1, 0), (4096, 2, 2, 0), (4096, 2, 5, 2), (4096, 2, 1024, 0), (1023, 1, 5, 0), (2047, 2, 5, 0), (2048, 2, 5, 0), (1 << 14, 2, 64, 0),
                (1 << 20, 1, 16, 0), (1, 2, 3, 0)):
        r, got = by_key[key], info(*key)
        assert got["batched"] and got["blobs_per_group"] == r["group"] and got["groups"] == -(-key[2] // r["group"]), key
        for a, b in (("c", "c"), ("W", "W"), ("G", "G"), ("entries", "entries"), ("nl", "nl"), ("seg", "seg"), ("sort_small", "small"), ("scan1", "scan1"),
                     ("launches", "launches"), ("workspace_bytes", "bytes")):
            assert got[a] == r[b], (key, a)
    # n = 4 096: one blob stays below the 2^18-entry sort switch, two are above it
    assert info(4096, 2, 1)["sort_small"] == 1 and info(4096, 2, 2)["sort_small"] == 0
    # the multi-kernel scan of the GPU test: 33 blobs of 2^14 scalars
    got = info(1 << 14, 2, 33)
    assert got["c"] == 8 and got["G"] == 33 * 32 * 128 and got["scan1"] == 0 and got["groups"] == 1
    # a blob above one launch goes alone (in parts)
    got = info((1 << 22) + 1, 2, 4)
    assert not got["batched"] and got["blobs_per_group"] == 1 and got["groups"] == 4
    # errors
    out = L.G2BatchInfo()
    assert lib.kzg_msm_g2_batch_info(16, 2, 4, 0, None) == L.ERR_INVALID_ARG
    assert lib.kzg_msm_g2_batch_info(16, 0, 4, 0, C.byref(out)) == L.ERR_INVALID_ARG
    assert lib.kzg_msm_g2_batch_info(16, 3, (1 << 20) + 1, 0, C.byref(out)) == L.ERR_INVALID_ARG          # nb before the count
    assert lib.kzg_msm_g2_batch_info(16, 2, (1 << 20) + 1, 0, C.byref(out)) == L.ERR_TOO_LARGE
    assert lib.kzg_msm_g2_batch_info(1 << 60, 2, 1 << 20, 0, C.byref(out)) == L.ERR_INVALID_ARG          # count n 32 overflows size_t
    assert lib.kzg_msm_g2_batch_info(16, 2, 1 << 20, 0, C.byref(out)) == L.OK and out.groups == -(-(1 << 20) // out.blobs_per_group)
    assert lib.kzg_msm_g2_batch_info(0, 2, 4, 0, C.byref(out)) == L.OK and out.groups == 0 and lib.kzg_msm_g2_batch_info(16, 2, 0, 0, C.byref(out)) == L.OK
    # the null and size rows of the batched calls need no device either
    assert lib.kzg_ctx_set_g2_batch_group(None, 2) == L.ERR_INVALID_ARG
    z = (C.c_uint64 * 16)()
    assert lib.kzg_msm_g2_srs_batch(None, None, 0, z, 1, 1, z, None) == L.ERR_INVALID_ARG
    assert lib.kzg_commit_with_length_proof_batch(None, None, None, None, 0, 16, z, 1, 1, 16, z, z, z) == L.ERR_INVALID_ARG
