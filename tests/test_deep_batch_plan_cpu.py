"""csrc/deep_batch_plan.hpp and gate_deep on the CPU (tests/native/deep_batch_plan_test.cpp, a stand-alone host program under
ASan + UBSan), and the C surface of the deep-k batch's switches without a device."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_and_gate(tmp_path):
    exe = tmp_path / "deep_batch_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "deep_batch_plan_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert re.search(r"\d+ plans and \d+ gates checked, 0 failures", r.stdout), r.stdout


def test_switches_on_a_null_handle_and_the_constant():
    import vectorlite_amd as V
    from vectorlite_amd import _lib
    L = _lib.load()
    assert L.vl_index_set_deep_batch(None, 1) == V.VL_ERR_INVALID_ARG
    assert L.vl_index_last_deep_batch(None, None) == V.VL_ERR_INVALID_ARG
    header = open(os.path.join(ROOT, "include", "vectorlite_amd.h")).read()
    assert re.search(r"#define VL_DEEP_MAX_K %d\b" % V.VL_DEEP_MAX_K, header)
