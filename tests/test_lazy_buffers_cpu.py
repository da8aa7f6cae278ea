"""csrc/lazy_buffers.hpp on the CPU: lazily made scratch buffers are all or nothing -- with a counting allocator that
fails each allocation index in turn, a fixed set of four and a grown pair end up null, without capacity and without a
live allocation, and the next call starts over."""
import os  # the native CPU tests run under AddressSanitizer + UBSan (sanitizers on the CPU build only)
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_failed_allocation_leaves_the_set_as_it_was_found(tmp_path):
    exe = tmp_path / "lazy_buffers_test"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "lazy_buffers_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "lazy buffers ok" in r.stdout


def test_the_header_has_no_hip_in_it():
    text = open(os.path.join(ROOT, "vectorlite_amd", "csrc", "lazy_buffers.hpp")).read()
    assert "hip" not in text.lower()
