"""csrc/masked_batch_plan.hpp on the CPU: the cost rule that sends a batch of exclusion-filtered queries to the mask-aware
MFMA pass or to the jobs kernel.  The native program checks properties R1-R5 of the header on random shapes (both
estimates monotone in the kept rows, the number of queries and the index length) and the named cases: the headline batch
(256 queries hiding 100 ids of 10 M x 384) takes the MFMA route, two queries keeping 0.1 % take the jobs route, an
ineligible input takes the MFMA route in no mode."""
import os  # the native CPU tests run under AddressSanitizer + UBSan (sanitizers on the CPU build only)
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_masked_batch_plan_rule(tmp_path):
    exe = tmp_path / "masked_batch_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "masked_batch_plan_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "masked batch plan ok" in r.stdout
