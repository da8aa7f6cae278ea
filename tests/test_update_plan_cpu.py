"""csrc/update_plan.hpp on the CPU: every plan of an in-place update / upsert, applied to a host mirror, leaves what the
sequential loop `contains(id) ? update(first row with id) : (insert_missing ? add : fail)` leaves; positions come out strictly
ascending, chunks fit the staging size, and a refusal names the loop's failing id and plans nothing."""
import os  # the native CPU tests run under AddressSanitizer + UBSan (sanitizers on the CPU build only)
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_update_plan_equals_the_sequential_loop(tmp_path):
    exe = tmp_path / "update_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), os.path.join(ROOT, "tests", "native", "update_plan_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "plans checked" in r.stdout
