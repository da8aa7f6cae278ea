"""tests/native/hnsw_graph_check.hpp on the CPU: the checker of the HNSW graph invariants G1 .. G8 (HNSW
section) names each invariant broken alone on a hand-made 12-node graph, passes the correct graph under all four metrics,
and its two restatements of the product -- the level law and the build's f32 edge key -- agree with values worked out by
hand and with a long-double evaluation."""
import os  # the native CPU tests run under AddressSanitizer + UBSan (sanitizers on the CPU build only)
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_checker_names_each_broken_invariant(tmp_path):
    exe = tmp_path / "hnsw_graph_check_test"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "hnsw_graph_check_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "hnsw graph check ok" in r.stdout


def test_the_checker_has_no_hip_in_it():
    text = open(os.path.join(ROOT, "tests", "native", "hnsw_graph_check.hpp")).read()
    assert "#include <hip" not in text and "__device__" not in text and "csrc" not in text
