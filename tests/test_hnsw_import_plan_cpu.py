"""vectorlite_amd/csrc/hnsw_import_plan.hpp on the CPU: the structural pass (G3, G4, list capacities) that every HNSW graph
import makes on the host before a device kernel sees a list.  tests/native/hnsw_import_plan_test.cpp is a stand-alone
program with hand-made graphs in exactly sized arrays; it names each violation with the graph audit's wording, in layer 0
and in an upper layer, at the first and the last slot, and reads nothing past a count, a node or a slot."""
import os  # the native CPU tests run under AddressSanitizer + UBSan (sanitizers on the CPU build only)
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "vectorlite_amd", "csrc", "hnsw_import_plan.hpp")


def test_the_import_plan_names_each_violation(tmp_path):
    exe = tmp_path / "hnsw_import_plan_test"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "hnsw_import_plan_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "hnsw import plan ok" in r.stdout


def test_the_import_plan_has_no_hip_and_no_product_state_in_it():
    text = open(HEADER).read()
    assert "#include <hip" not in text and "__device__" not in text and '#include "' not in text


def test_the_import_plan_words_its_violations_as_the_graph_audit_does():
    """The messages are restated, not shared (the audit is a test tool, the plan ships): the wording is pinned here."""
    plan = open(HEADER).read()
    audit = open(os.path.join(ROOT, "tests", "native", "hnsw_graph_check.hpp")).read()
    for phrase in ('" > capacity "', '" >= n"', '"a node lists itself"', '" listed above its level"', '" named twice"',
                   '" (node "', '", layer "', '", slot "'):
        assert phrase in plan and phrase in audit, phrase
