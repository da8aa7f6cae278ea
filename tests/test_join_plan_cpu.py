"""csrc/join_plan.hpp on the CPU: the similarity join's workgroup stretches cover every (row block, panel) unit of the
triangle exactly once with loads that differ by at most one unit, and its key threshold is monotone and minimal; and the
symmetry the join's contract leans on: the oracle scores (a, b) and (b, a) to the same bits for all four metrics."""
import os  # the native CPU tests run under AddressSanitizer + UBSan (sanitizers on the CPU build only)
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_join_plan_covers_the_triangle_once_and_threshold_is_monotone(tmp_path):
    exe = tmp_path / "join_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "join_plan_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "plans checked" in r.stdout


def test_oracle_scores_are_symmetric_and_the_join_symbols_exist():
    from oracle import oracle as O
    from vectorlite_amd import _lib
    assert {"vl_index_similarity_join", "vl_index_set_join_route", "vl_index_last_join"} <= set(_lib.SYMBOLS)
    O.build()
    rng = np.random.default_rng(29)
    for dim in (1, 3, 100, 384, 768):
        rows = rng.standard_normal((12, dim)) * rng.uniform(1e-3, 1e3, (12, 1))
        rows[3] = rows[2] * 1.5
        rows[5] = 0.0
        for metric in range(4):
            for i in range(12):
                for j in range(i, 12):
                    ab, ba = O.calculate(metric, rows[i], rows[j]), O.calculate(metric, rows[j], rows[i])
                    assert np.float64(ab).view(np.uint64) == np.float64(ba).view(np.uint64), (dim, metric, i, j, ab, ba)
