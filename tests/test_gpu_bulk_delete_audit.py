"""Audit of a flat index's device arrays and derived copies after bulk deletes (delete_many / vl_index_delete_bulk; DESIGN.md
§22, beside the derived-copies audit).

tests/native/bulk_delete_audit.hip drives GpuFlatIndex::remove_bulk in C++ with the compaction buffer at 16 KiB, keeps a plain
host mirror, and after every bulk delete compares the f32 slab (padding columns included), inv_norm, the device and host
flags and the out-of-domain count with the mirror's rows converted from row 0 by the library's own launchers; checks that
every copy's watermark is at or below the smallest removed position and that each lazily built copy equals the fresh
conversion below its watermark, and everywhere once it is built again.  Every comparison is of bytes or integers.
  a  a scripted stream (dim 100): holes at the edges of the index, of a 16-row fragment group and of a 64-row tile, below some
     watermarks and above others; a triple id; absent and repeated ids; every row; growth behind a compaction
  b  a seeded random stream (dim 128, 3000 rows): single ids, runs and random shares of 1 to 40 per cent, rows added between
"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def audit_exe(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    vbuild.build()  # the program links the library's objects: the private ensure_* members it calls
    d = tmp_path_factory.mktemp("bulk_delete_audit")
    exe, obj = d / "bulk_delete_audit", d / "bulk_delete_audit.o"
    arch = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"]
    objs = [os.path.join(vbuild.OBJ, os.path.splitext(s)[0] + ".o") for s in vbuild.SOURCES]
    for cmd in (arch + ["-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "bulk_delete_audit.hip"), "-o", str(obj)],
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


def test_scripted_holes_at_group_and_tile_edges(audit_exe):
    out = run_child([audit_exe, "a"], timeout=300)
    lines = summary_lines(out)
    print("\n" + "\n".join(lines))
    assert len(lines) == 1 and "dim=100" in lines[0], out[-2000:]
    # every scripted operation took its checkpoint: 2 builds, 14 bulk deletes, 2 adds
    assert int(lines[0].split(":")[1].split()[0]) == 18, lines


def test_seeded_random_stream(audit_exe):
    out = run_child([audit_exe, "b", "1"], timeout=300)
    lines = summary_lines(out)
    print("\n" + "\n".join(lines))
    assert len(lines) == 1 and "dim=128" in lines[0] and int(lines[0].split(":")[1].split()[0]) >= 25, out[-2000:]
