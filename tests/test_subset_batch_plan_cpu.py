"""csrc/subset_batch_plan.hpp on the CPU: which (query, filter) jobs of a filtered batch share a launch, and how wide.  The
native program checks invariants P1-P6 of the header on random job mixes and on the named examples (nine whole-index
filters, 256 filters of 10^4 and of 100 rows, one job, 513 jobs, three large filters among twenty small ones)."""
import os  # the native CPU tests run under AddressSanitizer + UBSan (sanitizers on the CPU build only)
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_subset_batch_plan_invariants(tmp_path):
    exe = tmp_path / "subset_batch_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "subset_batch_plan_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "plans checked" in r.stdout
