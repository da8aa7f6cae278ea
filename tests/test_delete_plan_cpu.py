"""csrc/delete_plan.hpp on the CPU: the bulk delete's segments tile the moved destinations once, a direct launch never
writes a row it has yet to read, a bounced segment fits the bounce, and every plan -- its launches' rows applied forward,
backward and shuffled -- leaves what std::remove_if leaves."""
import os  # the native CPU tests run under AddressSanitizer + UBSan (sanitizers on the CPU build only)
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_delete_plan_invariants_and_execution(tmp_path):
    exe = tmp_path / "delete_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), os.path.join(ROOT, "tests", "native", "delete_plan_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "plans checked" in r.stdout
