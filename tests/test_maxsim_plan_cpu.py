"""csrc/maxsim_plan.hpp on the CPU: the per-group upper bound's sum is at or above the long double sum of its terms and
monotone in every key (tests/native/maxsim_plan_test.cpp, a stand-alone host program under ASan + UBSan)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_maxsim_upper_bound_sum_is_safe_and_monotone(tmp_path):
    exe = tmp_path / "maxsim_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "maxsim_plan_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "sums checked, 0 failures" in r.stdout
