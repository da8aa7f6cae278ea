"""csrc/attr_plan.hpp on the CPU: the host half of an attribute column (sorted pairs, exact repeats dropped, conflicting
repeats rejected with the smallest id named, vl_index_attr_set's upsert, the size limit) against a std::map restatement."""
import os  # the native CPU tests run under AddressSanitizer + UBSan (sanitizers on the CPU build only)
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_attr_plan_matches_its_map_restatement(tmp_path):
    exe = tmp_path / "attr_plan_test"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "attr_plan_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "attr plan ok" in r.stdout


def test_the_plan_header_has_no_hip_in_it():
    text = open(os.path.join(ROOT, "vectorlite_amd", "csrc", "attr_plan.hpp")).read()
    assert "hip" not in text.split("#pragma once", 1)[1].lower()
