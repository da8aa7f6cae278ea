"""vectorlite_amd/csrc/hnsw_filter_plan.hpp on the CPU: the route (walk or exact) and the walk's list capacity of an
id-filtered HNSW search.  tests/native/hnsw_filter_plan_test.cpp is a stand-alone program that checks every boundary the
rule has -- no passing node, one, ef_walk 512 / 513, both sides of the 256 rule, every capacity step, products past
2^64 -- and sweeps a small domain against the rule restated without the 128-bit products."""
import os  # the native CPU tests run under AddressSanitizer + UBSan (sanitizers on the CPU build only)
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "vectorlite_amd", "csrc", "hnsw_filter_plan.hpp")


def test_the_filter_plan_routes_and_sizes_at_every_boundary(tmp_path):
    exe = tmp_path / "hnsw_filter_plan_test"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "hnsw_filter_plan_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "hnsw filter plan ok" in r.stdout


def test_the_filter_plan_has_no_hip_and_no_product_state_in_it():
    text = open(HEADER).read()
    assert "#include <hip" not in text and "__device__" not in text and '#include "' not in text


def test_the_index_plans_with_the_header_and_nothing_else():
    """hnsw_index.cpp takes route and capacity from the header: the constants appear nowhere else in the host code."""
    host = open(os.path.join(ROOT, "vectorlite_amd", "csrc", "hnsw_index.cpp")).read()
    assert '#include "hnsw_filter_plan.hpp"' in host and "hnsw_filter_plan(" in host
    assert "HNSW_FILTER_EXACT_RATIO" not in host
