"""Audit of HnswIndex::graph_import in C++ (DESIGN.md "Importing a graph").

tests/native/hnsw_graph_import_audit.hip builds an index with the batched GPU build, exports it, imports the arrays into a
fresh HnswIndex and copies the imported index's device arrays and host bookkeeping back.  tests/native/hnsw_graph_check.hpp
(G1 .. G9) must be clean on them with the source's orphan policy, and every array -- the edge distances dist0 / distU and
the in-degree counter indeg0 that the import's two kernels recompute among them -- must equal the source index's BITWISE over
the nodes and slots in use, with lock[] zero over the capacity.  Then a bulk add of 17 rows, a single add and three deletes
run on the imported index, the checker after each.
  a  n = 2060 across both capacity steps: euclidean dim 5 and cosine dim 100, ten tombstones, zero rows, 60 copies of one row
  b  (m, m0) = (4, 8) with manhattan and (48, 64) with the dot product, n = 600
  c  dim 3072, n = 300: the widest slab stride the distance routine serves
"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def audit_exe(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    vbuild.build()  # the program links the library's objects: the private members the probe reads
    d = tmp_path_factory.mktemp("hnsw_graph_import_audit")
    exe, obj = d / "hnsw_graph_import_audit", d / "hnsw_graph_import_audit.o"
    arch = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"]
    objs = [os.path.join(vbuild.OBJ, os.path.splitext(s)[0] + ".o") for s in vbuild.SOURCES]
    for cmd in (arch + ["-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "hnsw_graph_import_audit.hip"), "-o", str(obj)],
                arch + [str(obj)] + objs + vbuild.LINK + ["-o", str(exe)]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


_STATE = {"failed_child": None}


def run_child(args, timeout):
    """One audit child under its own time limit; after a child that did not exit cleanly no further one is started."""
    if _STATE["failed_child"]:
        pytest.fail(f"not started: the audit child {_STATE['failed_child']} failed")
    _STATE["failed_child"] = " ".join(args[1:])
    r = subprocess.run(args, capture_output=True, text=True, timeout=timeout)
    if r.returncode == 0 and "audit ok" in r.stdout:
        _STATE["failed_child"] = None
    else:
        pytest.fail(f"audit child exited {r.returncode}:\n{r.stdout[-6000:]}\n{r.stderr[-3000:]}")
    return r.stdout


def summary_lines(out):
    return [l for l in out.splitlines() if l.startswith("stream ")]


# source + imported + refused second import + bulk add + single add + three deletes
CHECKPOINTS = 8


def test_a_both_capacity_steps_tombstones_zero_rows_and_copies(audit_exe):
    lines = summary_lines(run_child([audit_exe, "a"], timeout=120))
    print("\n" + "\n".join(lines))
    assert len(lines) == 2 and "dim=5 metric=1 " in lines[0] and "dim=100 metric=0 " in lines[1], lines
    assert all(f": {CHECKPOINTS} checkpoints " in l and " n=2060 " in l and " orphans=0 " in l for l in lines), lines


def test_b_short_and_long_lists(audit_exe):
    lines = summary_lines(run_child([audit_exe, "b"], timeout=120))
    print("\n" + "\n".join(lines))
    assert len(lines) == 2 and "m=4 m0=8 metric=2 " in lines[0] and "m=48 m0=64 metric=3 " in lines[1], lines
    assert all(f": {CHECKPOINTS} checkpoints " in l and " n=600 " in l for l in lines), lines
    assert " orphans=0 " in lines[1], lines  # counted at m0 = 8, refused at m0 = 64


def test_c_dim_3072(audit_exe):
    lines = summary_lines(run_child([audit_exe, "c"], timeout=120))
    print("\n" + "\n".join(lines))
    assert len(lines) == 1 and f": {CHECKPOINTS} checkpoints " in lines[0] and " n=300 " in lines[0], lines
