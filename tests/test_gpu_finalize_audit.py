"""Audit of the list merge, finalize and selection launchers on synthetic lists.

Every fast search ends in launch_merge_finalize / launch_merge_finalize_multi / launch_batch_finalize, every exact one in
launch_exact_select; end to end they are only seen through answers, where a lost list shows only if it held a winner and
a wrong certification decision only on adversarial data.  tests/native/finalize_audit.hip hands hand-made sorted lists
(or a score array) to those launchers and dumps every byte they could have written; tests/_finalize_cases.py holds the
cases and the host model (shown right against FlatOracle by tests/test_finalize_model_cpu.py).  Here:
  * list counts 1 .. 4096 with winners planted in the first / last list of every group of 4 and block of 64,
  * the certification decision with the list's 64th key put exactly at tau(s_cut) (certified) and one f32 above (not),
    for every launcher, metric, in_extra and k in {1, 10, 60, 64}, and every branch of rank_check_emit,
  * rescoring at every width around the 48-column tile and the 384 / 192-column block, bitwise against the oracle,
  * the multi-partition finalize, and selection chains of up to SELECT_MAX_ROUNDS rounds.
No tolerance anywhere: bits and integers.  A query with a NaN score is judged on flags and n_out only (its ranking is
unspecified); no other query is skipped, and every test asserts that it judged as many queries as its cases hold.
k = 0 is accepted by the launchers (n_out = 0, no entry written) and is among the branch cases; the library's callers
never pass it: every FlatIndex search entry point returns an empty answer for k == 0 before a query is staged.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _finalize_cases as F  # noqa: E402
from oracle import oracle  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_STATE = {"failed_child": None}
COUNTS = {"cases": 0, "queries": 0, "decision pairs": 0, "select rounds": 0}


@pytest.fixture(scope="module")
def audit_exe(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    exe = tmp_path_factory.mktemp("finalize_audit") / "finalize_audit"
    cmd = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "finalize_audit.hip"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


@pytest.fixture(scope="module", autouse=True)
def count_report():
    yield
    print("\nfinalize audit judged: " + ", ".join(f"{v} {k}" for k, v in COUNTS.items()))


def run_child(args, what, ok):
    """One child at a time; once one has failed, hung or crashed no later case starts a process on the card."""
    if _STATE["failed_child"]:
        pytest.fail(f"not started: the audit child of {_STATE['failed_child']} failed")
    _STATE["failed_child"] = what  # cleared only on a clean exit: a timeout or a crash leaves it set
    r = subprocess.run(args, capture_output=True, text=True, timeout=180)
    if r.returncode == 0 and ok(r.stdout):
        _STATE["failed_child"] = None
    else:
        pytest.fail(f"audit child exited {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    return r.stdout


def run_file(exe, cases, tmp_path, bkeys=None):
    src, out = tmp_path / "cases.bin", tmp_path / "out.bin"
    F.write_cases(src, cases, bkeys)
    run_child([exe, str(src), str(out)], cases[0].name, lambda s: s.rstrip().endswith("audit ok"))
    return F.parse_output(out.read_bytes(), cases)


def tool_tau(exe, setups):
    """tau(s_cut) of every setup from the tool's host-only subcommand (range_tau of score_bound.hpp)."""
    args = [exe, "tau"]
    for s in setups:
        metric, ld, R, Q, sc, code = s.tau_request()
        args += [str(metric), str(ld)] + [format(int(F.bits(np.array([v]))[0]), "x") for v in (R, Q, sc)] + [str(code)]
    lines = run_child(args, "tau", lambda s: len(s.split()) == 2 * len(setups)).split("\n")
    taus = []
    for s, line in zip(setups, lines):
        found, b = line.split()
        tau = np.uint32(int(b, 16)).view(np.float32)
        assert found == "1" and np.isfinite(tau), (s.tau_request(), line)
        taus.append(tau)
    return taus


def judge_lists(exe, cases, tmp_path, shared_model=False):
    """Run list cases as one file and judge every query of every case.  shared_model: the cases differ only in their
    sink, so the merged candidates and their scores are computed once."""
    for c in cases:
        assert F.lists_sorted(c), (c.name, "the case itself is malformed")
    merged, answers = [], []
    for c in cases:
        if shared_model and merged:
            merged.append(merged[0])
            answers.append(answers[0])
        else:
            merged.append(F.merge_groups(c))
            answers.append(F.model_answers(c, oracle.calculate, merged[-1]))
    outs = run_file(exe, cases, tmp_path, [F.bound_requests(c, m) for c, m in zip(cases, merged)])
    want = judged = 0
    for c, m, a, o in zip(cases, merged, answers, outs):
        judged += F.judge_list_case(c, m, a, o)
        want += 0 if c.expect_refuse else (1 if c.mode == F.MULTI else c.nq)
    assert judged == want, ("queries judged", judged, "queries in the cases", want)
    COUNTS["cases"] += len(cases)
    COUNTS["queries"] += judged
    return merged, outs


def chunks(seq, n):
    return [tuple(seq[i:i + n]) for i in range(0, len(seq), n)]


# ---- 1. list counts ------------------------------------------------------------------------------------------------
COUNT_GROUPS = chunks([n for n in F.LIST_COUNTS if n <= 129], 4) + [(n,) for n in F.LIST_COUNTS if n > 129]


@pytest.mark.parametrize("counts", COUNT_GROUPS, ids=["-".join(map(str, g)) for g in COUNT_GROUPS])
def test_no_list_is_lost_at_any_list_count(audit_exe, counts, tmp_path):
    cases = []
    for n_lists in counts:
        cs = F.list_count_cases(n_lists)
        F.check_list_count_coverage(n_lists, cs, [F.merge_groups(c) for c in cs])  # on the host, before the device is judged
        cs[0].reuse_master = False
        cases += cs
    judge_lists(audit_exe, cases, tmp_path)


@pytest.mark.parametrize("nq,n_lists", F.BATCH_SHAPES, ids=[f"q{a}-L{b}" for a, b in F.BATCH_SHAPES])
def test_batch_shapes_with_and_without_a_sink(audit_exe, nq, n_lists, tmp_path):
    judge_lists(audit_exe, F.batch_shape_cases(nq, n_lists), tmp_path, shared_model=True)


# ---- 2. the decision -----------------------------------------------------------------------------------------------
def judge_pairs(exe, setups, tmp_path):
    taus = tool_tau(exe, setups)
    cases = [c for s, t in zip(setups, taus) for c in F.decision_pair(s, t)]
    for i, c in enumerate(cases):
        c.reuse_master = False
    merged, outs = judge_lists(exe, cases, tmp_path)
    for i, s in enumerate(setups):
        lo, hi = outs[2 * i], outs[2 * i + 1]
        # judge_list_case held the model's flags against expect_flags; the device's own, once more and by name
        assert int(lo["blocks"]["flags"][0]) == 0, (cases[2 * i].name, "key64 = tau must certify")
        assert int(hi["blocks"]["flags"][0]) == F.NEEDS_EXACT, (cases[2 * i + 1].name, "key64 = tau + 1 ulp must not certify")
        top = s.top if s.mode == F.MULTI else 0
        assert float(lo["B_dev"][top]) < s.s_cut <= float(hi["B_dev"][top]), (cases[2 * i].name, "tau does not bracket s_cut")
        COUNTS["decision pairs"] += 1


@pytest.mark.parametrize("metric", F.ALL4, ids=[F.METRIC_NAME[m] for m in F.ALL4])
@pytest.mark.parametrize("mode", (F.FINALIZE, F.BATCH), ids=["finalize", "batch"])
def test_decision_at_tau_and_one_ulp_above(audit_exe, mode, metric, tmp_path):
    setups = F.decision_setups(mode, metric, oracle.calculate)
    assert len(setups) == len(F.IN_EXTRA_CODES) * len(F.DECISION_KS)
    judge_pairs(audit_exe, setups, tmp_path)


def test_multi_decision_at_the_largest_partition_bound(audit_exe, tmp_path):
    judge_pairs(audit_exe, F.multi_decision_setups(oracle.calculate), tmp_path)


B_AT_ONE = {}


@pytest.mark.parametrize("mode", (F.FINALIZE, F.BATCH, F.MULTI), ids=["finalize", "batch", "multi"])
def test_a_score_equal_to_the_bound_is_not_certified(audit_exe, mode, tmp_path):
    if not B_AT_ONE:  # the device's B(key 1.0) per in_extra, from one probe file
        probe, bkeys = F.equality_probe()
        for c, o in zip(probe, run_file(audit_exe, probe, tmp_path, bkeys)):
            B_AT_ONE[c.code] = float(o["B_dev"][0])
    cases = F.equality_cases(mode, B_AT_ONE)
    merged, outs = judge_lists(audit_exe, cases, tmp_path)
    for c, o in zip(cases, outs):
        on = c.expect_flags[0] == F.NEEDS_EXACT
        for b in o["B_dev"]:  # the construction stands on the device's own bound: the planted score IS B, or the next f64
            assert (c.s_cut_planted == float(b)) if on else (c.s_cut_planted == float(np.nextafter(b, np.inf))), (c.name, b)
        assert int(o["blocks"]["flags"][0]) == c.expect_flags[0], c.name
    COUNTS["decision pairs"] += len(cases) // 2


@pytest.mark.parametrize("mode", (F.FINALIZE, F.BATCH), ids=["finalize", "batch"])
def test_branches_of_rank_check_emit(audit_exe, mode, tmp_path):
    judge_lists(audit_exe, F.branch_cases(mode), tmp_path)


# ---- 3. rescoring widths -------------------------------------------------------------------------------------------
WIDTH_GROUPS = [(F.FINALIZE, g) for g in chunks(F.FINALIZE_DIMS, 3)] + [(F.BATCH, g) for g in chunks(F.BATCH_DIMS, 3)]


@pytest.mark.parametrize("mode,dims", WIDTH_GROUPS, ids=[F.MODE_NAME[m] + "-" + "-".join(map(str, g)) for m, g in WIDTH_GROUPS])
def test_rescoring_is_the_oracle_bit_for_bit_at_every_width(audit_exe, mode, dims, tmp_path):
    judge_lists(audit_exe, [c for d in dims for c in F.width_cases(mode, d)], tmp_path)


# ---- 4. MULTI ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_parts", F.MULTI_PARTS)
def test_multi_partition_finalize(audit_exe, n_parts, tmp_path):
    judge_lists(audit_exe, [c for L in F.MULTI_L for c in F.multi_cases(n_parts, L)], tmp_path)


def test_multi_refuses_bad_partitions(audit_exe, tmp_path):
    judge_lists(audit_exe, F.multi_refusal_cases(), tmp_path)


# ---- 5. SELECT -----------------------------------------------------------------------------------------------------
SELECT_GROUPS = chunks(F.SELECT_N[:8], 4) + [F.SELECT_N[8:10], F.SELECT_N[10:11], F.SELECT_N[11:12]]


@pytest.mark.parametrize("ns", SELECT_GROUPS, ids=["-".join(map(str, g)) for g in SELECT_GROUPS])
def test_selection_rounds_chain_through_the_exact_order(audit_exe, ns, tmp_path):
    cases = [c for n in ns for c in F.select_cases(n)]
    outs = run_file(audit_exe, cases, tmp_path)
    for c, o in zip(cases, outs):
        COUNTS["select rounds"] += F.judge_select_case(c, o)
    COUNTS["cases"] += len(cases)
