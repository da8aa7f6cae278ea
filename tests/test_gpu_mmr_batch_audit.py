"""Audit of the batched diversified search's stage behind k_batch_rescore on inputs handed to it directly (DESIGN.md
section 27).

From outside (tests/test_gpu_mmr_batch.py) a query that the stage hands back without need is re-answered by the single call
and stays exact, and random rows never put a score ON the bound.  tests/native/mmr_batch_audit.hip feeds k_mmr_batch_rank and
k_mmr_batch_select hand-made lists, scores, master rows and query norms (n_cand 0 / 1 / 2 / 63 / 64; the bound above and
below every score, between ranks n - 1 and n, between ranks n - 2 and n - 1, a score exactly on it; equal scores with
positions out of order; identical rows; one NaN score; complete lists of m = 1 / 40 / 64 rows and m = 65; (k, fetch_k) =
(1, 1), (2, 2), (4, 20), (20, 20), (10, 60), (60, 60); lambda 0 / 0.25 / 0.5 / 1; dim 1 / 3 / 33 / 384 / 768; 1 / 5 / 131
queries; three metrics) and compares every word of every result block with its host model, which is built with
-ffp-contract=off, sums by index and evaluates bound_for_key from score_bound.hpp.
One child process at a time; after a child failed, crashed or timed out no later test starts one."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_STATE = {"failed_child": None}


@pytest.fixture(scope="module")
def audit_exe(tmp_path_factory):
    from vectorlite_amd import _lib, build as vbuild
    assert os.path.exists(_lib.SO_PATH), "the library is built before the tests run"
    d = tmp_path_factory.mktemp("mmr_batch_audit")
    exe, obj = d / "mmr_batch_audit", d / "mmr_batch_audit.o"
    arch = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"]
    lib_dir = os.path.dirname(_lib.SO_PATH)
    for cmd in (arch + ["-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "mmr_batch_audit.hip"), "-o", str(obj)],
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


def test_the_stage_against_its_host_model(audit_exe):
    out = run_child([audit_exe, "stage"], "stage")
    print(out)
    # 3 metrics x 6 (k, fetch_k) x 5 sizes of S x (1 + 5 + 131) queries; lambda and dim rotate through the launches
    assert "mmr batch: 12330 queries in 270 launches, 0 mismatches" in out
