"""csrc/examples_plan.hpp on the CPU (tests/native/examples_plan_test.cpp, a stand-alone host program under ASan + UBSan): the
per-example map and the upper bound U against their long double restatements, U weakly increasing, the column layout,
gate_examples against its condition; and the C surface of vl_index_search_examples without a device."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_map_bound_layout_and_gate(tmp_path):
    exe = tmp_path / "examples_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "examples_plan_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "12000 example sets checked, 0 failures" in r.stdout


def test_examples_symbols_and_limits():
    from vectorlite_amd import _lib
    names = {"vl_index_search_examples", "vl_index_last_examples"}
    assert names <= set(_lib.SYMBOLS)
    header = open(os.path.join(ROOT, "include", "vectorlite_amd.h")).read()
    for name in names:
        assert re.search(r"\bint %s\(" % name, header), name
    assert re.search(r"#define VL_EXAMPLES_MAX_POS 64\b", header) and re.search(r"#define VL_EXAMPLES_MAX_NEG 32\b", header)


def test_argument_checks_answer_on_a_null_handle():
    import vectorlite_amd as V
    from vectorlite_amd import _lib
    L = _lib.load()
    n = C.c_uint64(7)
    for n_pos, n_neg, word in ((0, 0, b"VL_EXAMPLES_MAX_POS"), (65, 0, b"VL_EXAMPLES_MAX_POS"), (1, 33, b"VL_EXAMPLES_MAX_NEG")):
        # the example counts are checked before the handle, the positives' before the negatives', both before the metric
        assert L.vl_index_search_examples(None, None, n_pos, None, n_neg, 4, 1, 9, 0, None, None, C.byref(n)) == V.VL_ERR_INVALID_ARG
        assert n.value == 0 and word in L.vl_last_error()
    assert L.vl_index_search_examples(None, None, 1, None, 0, 4, 1, 9, 0, None, None, C.byref(n)) == V.VL_ERR_INVALID_ARG
    assert b"metric" in L.vl_last_error()
    assert L.vl_index_search_examples(None, None, 1, None, 0, 4, 1, 0, 0, None, None, C.byref(n)) == V.VL_ERR_INVALID_ARG
    assert L.vl_index_last_examples(None, None) == V.VL_ERR_INVALID_ARG
