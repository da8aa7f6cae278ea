"""csrc/group_plan.hpp on the CPU: the host half of a group table (sorted pairs, conflicting repeats rejected, distinct keys
numbered densely) against a std::map restatement."""
import os  # the native CPU tests run under AddressSanitizer + UBSan (sanitizers on the CPU build only)
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_plan_matches_its_map_restatement(tmp_path):
    exe = tmp_path / "group_plan_test"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "group_plan_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "group plan ok" in r.stdout


def test_the_plan_header_has_no_hip_in_it():
    text = open(os.path.join(ROOT, "vectorlite_amd", "csrc", "group_plan.hpp")).read()
    assert "hip" not in text.split("#pragma once", 1)[1].lower()
