"""Audit of the batched grouped search's two kernels on inputs handed to them directly.

From outside (tests/test_gpu_grouped_batch.py) a query that the collapse stage hands back without need is re-answered by the
single call and stays exact, and random rows never put a score ON the bound.  tests/native/grouped_batch_audit.hip
  1. feeds k_batch_rank_collapse hand-made lists, scores and group tables (n_cand 0 / 1 / 63 / 64; one group, own groups,
     groups of 2-5; the bound above, below and between the ranks, a score exactly on it; equal scores with positions out of
     order; one NaN; a complete list of 1 / 40 / 64 rows with fewer than k groups; n_rows = 65; k 1 / 10 / 60; 1 / 5 / 131
     queries; three metrics) and compares every word of every result block with its host model, which evaluates
     bound_for_key from score_bound.hpp;
  2. runs k_group_keep_bits on the cases built here; bitmap, count, the zero bits past `len` and two guard words are compared
     with numpy.
One child process at a time; after a child failed, crashed or timed out no later test starts one."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
GUARD = 0xA5A5A5A5A5A5A5A5

_STATE = {"failed_child": None}


@pytest.fixture(scope="module")
def audit_exe(tmp_path_factory):
    from vectorlite_amd import _lib, build as vbuild
    assert os.path.exists(_lib.SO_PATH), "the library is built before the tests run"
    d = tmp_path_factory.mktemp("grouped_batch_audit")
    exe, obj = d / "grouped_batch_audit", d / "grouped_batch_audit.o"
    arch = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"]
    lib_dir = os.path.dirname(_lib.SO_PATH)
    for cmd in (arch + ["-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "grouped_batch_audit.hip"), "-o", str(obj)],
                arch + [str(obj), "-L", lib_dir, "-lvectorlite_amd", f"-Wl,-rpath,{lib_dir}", "-o", str(exe)]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


def run_child(args, what):
    if _STATE["failed_child"]:
        pytest.fail(f"not started: the audit child of {_STATE['failed_child']} failed")
    _STATE["failed_child"] = what  # cleared only on a clean exit: a timeout or a crash leaves it set
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    if r.returncode == 0 and r.stdout.rstrip().endswith("audit ok"):
        _STATE["failed_child"] = None
    else:
        pytest.fail(f"audit child exited {r.returncode}:\n{r.stdout[-4000:]}\n{r.stderr[-3000:]}")
    return r.stdout


def test_the_collapse_stage_against_its_host_model(audit_exe):
    out = run_child([audit_exe, "collapse"], "collapse")
    print(out)
    assert "collapse: 6165 queries in 135 launches, 0 mismatches" in out  # 3 metrics x 3 k x 5 n_rows x (1 + 5 + 131)


# ---- k_group_keep_bits against numpy -----------------------------------------------------------------------------------
LENGTHS = (1, 63, 64, 65, 8191)
TABLES = ("all", "none", "alternate")
FILTERS = ("table only", "exclusion bitmap", "include ids")


def keep_case(rng, n, table, flt):
    gor = np.full(n, NONE, dtype=np.uint32)
    if table == "all":
        gor[:] = rng.integers(0, max(n // 3, 1), n, dtype=np.uint32)
    elif table == "alternate":
        gor[::2] = rng.integers(0, max(n // 3, 1), gor[::2].size, dtype=np.uint32)
    words = (n + 63) // 64
    case = {"n": n, "gor": gor, "mode": FILTERS.index(flt)}
    expect = gor != NONE
    if flt == "exclusion bitmap":
        kept = rng.random(n) < 0.6
        bits = np.zeros(words * 64, dtype=bool)
        bits[:n] = kept
        case["fkeep"] = np.packbits(bits.reshape(words, 64), axis=1, bitorder="little").view(np.uint64).ravel()
        expect = expect & kept
    elif flt == "include ids":
        pos_ids = (rng.permutation(n).astype(np.uint64) * np.uint64(7919) + np.uint64(3)) % np.uint64(2 ** 40)
        pos_ids[n // 2:n // 2 + 2] = pos_ids[0]  # duplicate-id rows all follow their id
        chosen = np.unique(pos_ids[rng.random(n) < 0.4])
        fids = np.unique(np.concatenate([chosen, np.array([2 ** 41, 2 ** 41 + 5], dtype=np.uint64)]))  # and ids no row has
        case["pos_ids"], case["fids"] = pos_ids, fids
        expect = expect & np.isin(pos_ids, chosen)
    case["expect"] = expect
    return case


def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(np.uint64(len(cases)).tobytes())
        for c in cases:
            nf = len(c["fids"]) if c["mode"] == 2 else 0
            f.write(np.array([c["n"], c["mode"], nf], dtype=np.uint64).tobytes())
            gor = c["gor"] if c["n"] % 2 == 0 else np.concatenate([c["gor"], np.zeros(1, dtype=np.uint32)])
            f.write(gor.tobytes())
            if c["mode"] == 1:
                f.write(c["fkeep"].tobytes())
            if c["mode"] == 2:
                f.write(c["pos_ids"].tobytes())
                f.write(c["fids"].tobytes())


def test_the_keep_bitmap_against_numpy(audit_exe, tmp_path):
    rng = np.random.default_rng(26)
    cases = [keep_case(rng, n, t, f) for n in LENGTHS for t in TABLES for f in FILTERS]
    # an include token with an empty id set keeps nothing
    empty = keep_case(rng, 65, "all", "include ids")
    empty["fids"] = np.zeros(0, dtype=np.uint64)
    empty["expect"] = np.zeros(65, dtype=bool)
    cases.append(empty)
    src, out = tmp_path / "cases.bin", tmp_path / "out.bin"
    write_cases(src, cases)
    run_child([audit_exe, "keepbits", str(src), str(out)], "keepbits")
    raw = np.frombuffer(out.read_bytes(), dtype=np.uint64)
    at, judged, set_bits = 0, 0, 0
    for c in cases:
        m, words = int(raw[at]), int(raw[at + 1])
        assert words == (c["n"] + 63) // 64
        keep = raw[at + 2:at + 2 + words]
        guard = raw[at + 2 + words:at + 4 + words]
        at += 4 + words
        bits = np.unpackbits(keep.view(np.uint8), bitorder="little").astype(bool)
        what = (c["n"], c["mode"])
        assert guard.tolist() == [GUARD, GUARD], what
        assert not bits[c["n"]:].any(), what  # bits at or past len are 0
        assert np.array_equal(bits[:c["n"]], c["expect"]), what
        assert m == int(c["expect"].sum()), what
        judged += 1
        set_bits += m
    assert at == raw.size and judged == len(LENGTHS) * len(TABLES) * len(FILTERS) + 1
    assert set_bits > 10_000  # the cases are not all empty
