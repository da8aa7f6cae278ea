"""csrc/assign_plan.hpp on the CPU (tests/native/assign_plan_test.cpp, a stand-alone host program under ASan + UBSan): the
second pass' f32 keep test never drops a pair whose bound reaches the seed score, the row ranges cover every block once
through splits, gate_assign reads each of its terms; and the C surface of vl_index_assign without a device."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keep_test_is_safe_ranges_cover_once_and_gate_reads_its_terms(tmp_path):
    exe = tmp_path / "assign_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "assign_plan_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "range plans checked, 0 failures" in r.stdout


def test_assign_symbols_and_limit():
    from vectorlite_amd import _lib
    names = {"vl_index_assign", "vl_index_set_assign_route", "vl_index_last_assign"}
    assert names <= set(_lib.SYMBOLS)
    header = open(os.path.join(ROOT, "include", "vectorlite_amd.h")).read()
    for name in names:
        assert re.search(r"\bint %s\(" % name, header), name
    assert re.search(r"#define VL_ASSIGN_MAX_LABELS 4096\b", header)


def test_argument_checks_answer_on_a_null_handle():
    import vectorlite_amd as V
    from vectorlite_amd import _lib
    L = _lib.load()
    n = C.c_uint64(7)
    for n_labels in (0, 4097):  # the label count is checked before the handle
        assert L.vl_index_assign(None, None, n_labels, 4, 0, 0, None, None, None, C.byref(n)) == V.VL_ERR_INVALID_ARG
        assert n.value == 0 and b"VL_ASSIGN_MAX_LABELS" in L.vl_last_error()
    assert L.vl_index_assign(None, None, 1, 4, 9, 0, None, None, None, C.byref(n)) == V.VL_ERR_INVALID_ARG
    assert b"metric" in L.vl_last_error()
    assert L.vl_index_assign(None, None, 1, 4, 0, 0, None, None, None, C.byref(n)) == V.VL_ERR_INVALID_ARG
    assert L.vl_index_set_assign_route(None, 0) == V.VL_ERR_INVALID_ARG
    assert L.vl_index_last_assign(None, None) == V.VL_ERR_INVALID_ARG
