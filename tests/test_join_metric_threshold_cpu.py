"""csrc/join_plan.hpp's per-pair thresholds for the Euclidean and dot similarity joins, on the CPU under ASan + UBSan
(tests/native/join_metric_threshold_test.cpp): monotone bound, cautious launch scalar, the kernel's f32 test never rejects."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_thresholds_are_monotone_cautious_and_never_reject(tmp_path):
    exe = tmp_path / "join_metric_threshold_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "join_metric_threshold_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.returncode, r.stdout, r.stderr)
