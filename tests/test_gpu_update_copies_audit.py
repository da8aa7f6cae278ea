"""Audit of every device copy a flat index derives from its f64 master rows, after in-place updates and upserts
(vl_index_update / vl_index_update_bulk).

tests/native/update_copies_audit.hip drives GpuFlatIndex in C++, keeps a plain host mirror of it, and after every operation
compares the index -- master, f32 slab, inv_norm, flags, both bf16 copies with norm16 / sqnorm, the int8 copy with (s, r) and
|row|, the watermarks, row_flags_, n_out_of_domain_, mutations_ -- with the mirror's rows converted from row 0 by the
library's own launchers.  Every comparison is of bytes or integers.  A search cannot see a stale row of a copy unless its
true top k holds that very row; this can.
  a  boundaries and watermarks (dim 100 and 384, 2100 rows): positions 0, 15, 16, 31, 32, 63, 64, the last rows of the last
     whole and of the partial 16-row group; no lazy copy, each one alone, all of them; rows below, at and above each
     watermark; in the domain -> out of it -> back, a zero row, a tiny row; an id stored three times; refused calls; a
     two-row staging buffer under a 40-row update and an upsert
  b  a seeded random stream (dim 128, 3000 rows, 150 operations: update, bulk update, upsert, add, delete, delete_many,
     clone, with builds of random subsets of the copies in between)
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
    d = tmp_path_factory.mktemp("update_copies_audit")
    exe, obj = d / "update_copies_audit", d / "update_copies_audit.o"
    arch = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"]
    objs = [os.path.join(vbuild.OBJ, os.path.splitext(s)[0] + ".o") for s in vbuild.SOURCES]
    for cmd in (arch + ["-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "update_copies_audit.hip"), "-o", str(obj)],
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


def summary(line):
    """'stream a dim=100: 55 checkpoints, 40 updates, rows rewritten per copy 1 / 2 / 3, ...' -> (55, 40, [1, 2, 3])"""
    body = line.split(":", 1)[1]
    ckpt, updates = int(body.split("checkpoints")[0]), int(body.split("checkpoints,")[1].split("updates")[0])
    per_copy = [int(x) for x in body.split("per copy")[1].split(",")[0].split("/")]
    return ckpt, updates, per_copy


def test_boundaries_and_watermarks(audit_exe):
    out = run_child([audit_exe, "a"], timeout=300)
    lines = [l for l in out.splitlines() if l.startswith("stream ")]
    print("\n" + "\n".join(lines))
    assert len(lines) == 2 and "dim=100" in lines[0] and "dim=384" in lines[1], out[-2000:]
    for l in lines:
        ckpt, updates, per_copy = summary(l)
        # every scripted operation took its checkpoint (5 + 3 x 7 + 16 + 6 + 3 + 2 + 2), 41 of them behind an update call,
        # and every lazy copy had rows rewritten in it
        assert ckpt == 55 and updates == 41 and all(c > 0 for c in per_copy), l


def test_seeded_random_stream(audit_exe):
    out = run_child([audit_exe, "b", "1"], timeout=300)
    lines = [l for l in out.splitlines() if l.startswith("stream ")]
    print("\n" + "\n".join(lines))
    assert len(lines) == 1, out[-2000:]
    ckpt, updates, per_copy = summary(lines[0])
    assert ckpt == 151 and updates >= 40 and all(c > 0 for c in per_copy), lines[0]  # 5 of 9 operation kinds are updates
