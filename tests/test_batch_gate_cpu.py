"""csrc/batch_gate.hpp on the CPU: for every combination of small domains of its inputs, each MFMA route's gate function
against that route's condition, restated independently in the native test."""
import os  # the native CPU tests run under AddressSanitizer + UBSan (sanitizers on the CPU build only)
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_each_route_decides_as_its_own_condition(tmp_path):
    exe = tmp_path / "batch_gate_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "batch_gate_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "gate decisions checked, 0 failures" in r.stdout
