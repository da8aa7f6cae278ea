"""Audit of the attribute-column and predicate-filter resolution kernels alone (csrc/where.hip).

tests/native/where_audit.hip drives launch_attr_rows, launch_where_bits and launch_where_compact on synthetic columns -- no
index, no slab -- and compares value_of_row, the has-bitmap, the row count, the keep words, the chunk offsets, m and the
position list with a host model, integer for integer:
  n           1, 63, 64, 65, 127, 128, 4133 (one child), 1 048 576 and 1 100 003, where chunks stop being 1024 rows (another)
  values      INT64_MIN, -1, 0, 1, INT64_MAX among others
  predicates  lo == hi, lo > hi, the full range, middle ranges; each plain and negated
  clauses     one to four, over distinct columns and over one column twice
  has-bitmaps all ones (also past n), all zeros, alternating words, only the last valid bit, a random 70 %
  tail        value_of_row holds garbage at and past n: it survives the column resolution and never reaches a keep bit
"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def audit_exe(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    so = vbuild.build()  # the program calls the library's launchers
    d = tmp_path_factory.mktemp("where_audit")
    exe = d / "where_audit"
    cmd = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}", "-O2", "-std=c++17", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "where_audit.hip"), f"-L{os.path.dirname(so)}", "-lvectorlite_amd",
           f"-Wl,-rpath,{os.path.dirname(so)}"] + vbuild.LINK + ["-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


_STATE = {"failed_child": None}


def run_child(args, timeout):
    """One audit child; after a child that did not exit cleanly no further one is started."""
    if _STATE["failed_child"]:
        pytest.fail(f"not started: the audit child {_STATE['failed_child']} failed")
    _STATE["failed_child"] = " ".join(args[1:])
    r = subprocess.run(args, capture_output=True, text=True, timeout=timeout)
    if r.returncode == 0 and "audit ok" in r.stdout:
        _STATE["failed_child"] = None
    else:
        pytest.fail(f"audit child exited {r.returncode}:\n{r.stdout[-6000:]}\n{r.stderr[-3000:]}")
    return r.stdout


def case_lines(out):
    return [l for l in out.splitlines() if l.startswith("case n=")]


def test_small_sizes_around_the_word_edges(audit_exe):
    lines = case_lines(run_child([audit_exe, "small"], timeout=300))
    print("\n" + "\n".join(lines))
    assert [int(l.split("=")[1].split(":")[0]) for l in lines] == [1, 63, 64, 65, 127, 128, 4133]
    assert all(int(l.split(":")[1].split()[0]) == 5 * 14 + 8 for l in lines), lines  # every predicate run took place


def test_sizes_where_chunks_stop_being_1024_rows(audit_exe):
    lines = case_lines(run_child([audit_exe, "big"], timeout=300))
    print("\n" + "\n".join(lines))
    assert [int(l.split("=")[1].split(":")[0]) for l in lines] == [1048576, 1100003]
    assert all(int(l.split(":")[1].split()[0]) == 5 * 14 + 8 for l in lines), lines
