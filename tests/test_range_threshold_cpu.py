"""csrc/score_bound.hpp on the CPU: the host routine that turns a range search's score threshold into a threshold on scan
keys (range_tau), against the host build of the shipped bound_for_key; and the bound's weak monotonicity in the key."""
import os  # the native CPU tests run under AddressSanitizer + UBSan (sanitizers on the CPU build only)
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tau_is_the_largest_key_whose_bound_is_below_the_threshold(tmp_path):
    exe = tmp_path / "range_threshold_test"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "range_threshold_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "range thresholds ok" in r.stdout


def test_kernels_take_the_bound_from_the_shared_header():
    """One definition: kernels.hip includes the header and defines no bound of its own."""
    csrc = os.path.join(ROOT, "vectorlite_amd", "csrc")
    hip = open(os.path.join(csrc, "kernels.hip")).read()
    assert '#include "score_bound.hpp"' in hip
    assert "double bound_for_key(" not in hip
    assert open(os.path.join(csrc, "score_bound.hpp")).read().count("double bound_for_key(") == 1
