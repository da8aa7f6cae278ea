"""csrc/where_plan.hpp on the CPU: the word-aligned chunking of a predicate resolution and the list / masked-ladder route
of a single search under a predicate token (properties C1, C2, W1..W6 of the header; the crossover at ld = 384)."""
import os  # the native CPU tests run under AddressSanitizer + UBSan (sanitizers on the CPU build only)
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_where_plan_properties(tmp_path):
    exe = tmp_path / "where_plan_test"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "where_plan_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "where plan ok" in r.stdout


def test_the_plan_header_has_no_hip_in_it():
    text = open(os.path.join(ROOT, "vectorlite_amd", "csrc", "where_plan.hpp")).read()
    assert "hip" not in text.split("#pragma once", 1)[1].lower()
