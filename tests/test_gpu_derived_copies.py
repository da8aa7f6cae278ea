"""Audit of every device copy a flat index derives from its f64 master rows, after add / delete / truncate streams
(beside the filter audits).

tests/native/derived_copies_audit.hip drives GpuFlatIndex in C++, keeps a plain host mirror of it, and after every mutation
compares the index's incremental state -- the f32 slab, inv_norm, the flags, both bf16 copies with their per-row arrays,
the int8 copy, the device id table, two id filters' and a group table's resolved lists, and the host bookkeeping -- with the
mirror's rows converted from row 0 by the library's own launchers.  Every comparison is of bytes or integers; only the largest
row norm may stay high after a delete.  The searches-after-mutations tests cannot see a stale row of a copy: a key that is
too high only costs a candidate, one that is too low matters only to a query whose true top k holds that very row.
  a  watermarks and boundaries (dim 100 and 384): growth across 1024 and 2048, deletes at the edges of the index, of a
     16-row fragment group and of a 64-row MFMA tile after builds of some copies only, a triple id, truncate, rows outside
     the fast-path domain, refused adds
  b  a seeded random stream (dim 128, 3000 rows, 150 operations, clones and truncates among them)
  c  the delete's bounce loop (9000 x 1000: the first move of more than one 64 MB chunk in the suite)
"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def audit_exe(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    vbuild.build()  # the program links the library's objects: the private ensure_* / resolve_* members it calls
    d = tmp_path_factory.mktemp("derived_copies_audit")
    exe, obj = d / "derived_copies_audit", d / "derived_copies_audit.o"
    arch = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"]
    objs = [os.path.join(vbuild.OBJ, os.path.splitext(s)[0] + ".o") for s in vbuild.SOURCES]
    for cmd in (arch + ["-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "derived_copies_audit.hip"), "-o", str(obj)],
                arch + [str(obj)] + objs + vbuild.LINK + ["-o", str(exe)]):
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


def summary_lines(out):
    return [l for l in out.splitlines() if l.startswith("stream ")]


def test_watermarks_and_boundaries(audit_exe):
    out = run_child([audit_exe, "a"], timeout=300)
    lines = summary_lines(out)
    print("\n" + "\n".join(lines))
    assert len(lines) == 2 and "dim=100" in lines[0] and "dim=384" in lines[1], out[-2000:]
    # every scripted mutation took its checkpoint: 30 + 20 + 5 + 4 single adds, 5 x 7 boundary deletes, ...
    assert all(int(l.split(":")[1].split()[0]) >= 180 for l in lines), lines


def test_seeded_random_stream(audit_exe):
    out = run_child([audit_exe, "b", "1"], timeout=300)
    lines = summary_lines(out)
    print("\n" + "\n".join(lines))
    assert len(lines) == 1 and int(lines[0].split(":")[1].split()[0]) >= 120, out[-2000:]


def test_delete_moves_more_than_one_bounce_chunk(audit_exe):
    out = run_child([audit_exe, "c"], timeout=300)
    lines = summary_lines(out)
    print("\n" + "\n".join(lines))
    assert len(lines) == 1 and int(lines[0].split(":")[1].split()[0]) == 4, out[-2000:]
