"""Audit of the batched range search's device stages on inputs handed to them directly (DESIGN.md sections 6 and 17).

From outside (tests/test_gpu_range_batch.py) a query whose counter passes the capacity, whose NaN flag is set or whose
`want` comes out 0 is re-answered by the single call and is still exact: a pass that marks overflow when nothing
overflowed, a tail that drops `want` to 0, a ring flush that loses entries but also marks, or a threshold computed with too
small an input-rounding term all stay green there.  tests/native/range_batch_audit.hip runs launch_rows_bf16_frag +
launch_mfma_range_candidates and launch_range_batch_tail on the cases of tests/_range_batch_cases.py and dumps every buffer
whole, guards included; the judges there compare with host models (tests/test_range_batch_model_cpu.py shows the tail
model right against FlatOracle and checks every construction's preconditions).
  1. the pass on lattice data, where keys are exact in any order: every stride, chunk boundary, row-count tail, grid and
     load form; thresholds ON a key (tie in) and on its successor (out); sets, key bits and counters at zero tolerance;
  2. the pass on rounded inputs: thresholds in gaps no row's allowance reaches, the certificate on both sides of the
     threshold, and bit consistency of the keys between two runs under another grid and load form;
  3. planted pairs that spend the bf16 slack: candidates under IN_EXTRA_MFMA, missed under IN_EXTRA_BF16_SINGLE;
  4. the ring segment filled exactly and by one block too many, carried over a block, and small candidate buffers;
  5. the tail on synthetic candidate lists, bits and integers against the model;
  6. pass and tail chained on one set of buffers against the oracle's range answers.
One child process at a time; after a child failed, crashed or timed out no later case starts one.  Every test asserts
how many (case, query) pairs it judged.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _range_batch_cases as RB  # noqa: E402
from oracle import oracle  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_STATE = {"failed_child": None}
COUNTS = {"pass queries": 0, "pass queries compared entry by entry": 0, "rerun queries": 0, "planted pairs": 0, "ring queries": 0, "of them marked in the mixed case": 0, "tail queries": 0, "chain queries": 0}
SHARE = {}  # (metric, stride) -> largest share of the bound a planted pair used


@pytest.fixture(scope="module")
def audit_exe(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    vbuild.build()  # the MFMA launchers: mfma_scan.o of the library build
    d = tmp_path_factory.mktemp("range_batch_audit")
    exe, obj = d / "range_batch_audit", d / "range_batch_audit.o"
    arch = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"]
    for cmd in (arch + ["-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "range_batch_audit.hip"), "-o", str(obj)],
                arch + [str(obj), os.path.join(vbuild.OBJ, "mfma_scan.o"), "-o", str(exe)]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


@pytest.fixture(scope="module", autouse=True)
def count_report():
    yield
    print("\nrange batch audit judged: " + ", ".join(f"{v} {k}" for k, v in COUNTS.items()))
    for (m, ld), s in sorted(SHARE.items()):
        print(f"  largest share of the bound used by a planted pair, {RB.METRIC_NAME[m]:9s} stride {ld}: {s:.4f}")


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


def run_file(exe, cases, tmp_path, tag=""):
    src, out = tmp_path / f"cases{tag}.bin", tmp_path / f"out{tag}.bin"
    RB.write_cases(src, cases)
    run_child([exe, str(src), str(out)], cases[0].name, lambda s: s.rstrip().endswith("audit ok"))
    return RB.parse_output(out.read_bytes(), cases)


def tool_thr(exe, requests):
    """range_key_threshold of every (metric, ldb, R, Q, min_score, in_extra) from the tool's host-only subcommand."""
    args = [exe, "thr"]
    for metric, ldb, R, Q, ms, ie in requests:
        args += [str(metric), str(ldb)] + [format(int(RB.bits64(np.array([v]))[0]), "x") for v in (R, Q, ms, ie)]
    lines = run_child(args, "thr", lambda s: len(s.split()) == 2 * len(requests)).strip().split("\n")
    out = []
    for line in lines:
        code, b = line.split()
        out.append((int(code), np.uint32(int(b, 16)).view(np.float32)))
    return out


# ---- 1. the pass on lattice data, every shape --------------------------------------------------------------------------
@pytest.mark.parametrize("dim", RB.PASS_DIMS)
def test_pass_lists_exactly_the_rows_at_or_above_the_threshold(audit_exe, dim, tmp_path):
    shapes = RB.lattice_shapes(dim)
    cases = [RB.lattice_case(dim, *shape) for shape in shapes]
    # the shapes whose chunks hold more than the ring does at the ranks above, again at ranks it holds
    light = [RB.lattice_case(dim, *shape, ranks=RB.light_ranks(shape[0])) for shape in shapes if shape[1] > 2]
    cases += light
    outs = run_file(audit_exe, cases, tmp_path)
    judged = exact = 0
    for c, o in zip(cases, outs):
        j, e = RB.judge_lattice(c, o)
        judged, exact = judged + j, exact + e
        if any(c is x for x in light):
            assert e == j, (c.name, "the light ranks must not overflow a segment", e, j)
    assert judged == sum(c.nq * len(c.metrics) * 2 for c in cases)
    COUNTS["pass queries"] += judged
    COUNTS["pass queries compared entry by entry"] += exact


# ---- 2. rounded inputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", RB.ROUNDED_DIMS)
def test_pass_on_rounded_inputs_certifies_and_keys_do_not_depend_on_the_launch(audit_exe, dim, tmp_path):
    cases = [RB.rounded_case(fam, dim) for fam in RB.ROUNDED_FAMILIES]  # one workgroup, streaming loads
    outs = run_file(audit_exe, cases, tmp_path)
    judged = 0
    for c, o in zip(cases, outs):
        j, _ = RB.judge_rounded(c, o)
        judged += j
    assert judged == sum(c.nq * len(c.metrics) for c in cases)
    COUNTS["pass queries"] += judged
    # (d) the keys of (row, query) under the default grid and plain loads are the first run's, bit for bit
    again = [RB.rerun_case(c, o, grid=0, stream=0) for c, o in zip(cases, outs)]
    outs2 = run_file(audit_exe, again, tmp_path, "2")
    rejudged = sum(RB.judge_rerun(c, o) for c, o in zip(again, outs2))
    assert rejudged == 2 * judged
    COUNTS["rerun queries"] += rejudged


# ---- 3. the edge of the bf16 slack -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", RB.EDGE_DIMS)
def test_threshold_is_sound_where_both_roundings_lose_a_full_unit(audit_exe, dim, tmp_path):
    """Planted (row, query) pairs whose bf16 copies lose 0.00775 of the product (the limit for two roundings is 0.00777;
    EDGE_LOSS = 0.0075 is reached at every stride).  With min_score = the planted row's exact score the row must be a
    candidate under thr(IN_EXTRA_MFMA) and -- the negative control -- must NOT be one under thr(IN_EXTRA_BF16_SINGLE)."""
    case = RB.edge_case(dim)
    planted = case.note["planted"]
    R = float(np.sqrt(RB.dev_sumsq(case.rows)).max())
    Q = [RB.seq_norm(q) for q in case.queries]
    requests = []
    for m in case.metrics:
        for exact, part in RB.edge_product_and_key(case, m):  # precondition, on the host
            assert 0.0 < part <= (1.0 - RB.EDGE_LOSS) * exact, (case.name, m, part, exact)
        ms = [oracle.calculate(m, case.rows[p], case.queries[j]) for j, p in enumerate(planted)]
        case.min_scores[m] = ms
        for ie in (RB.IN_EXTRA_MFMA, RB.IN_EXTRA_BF16_SINGLE):
            requests += [(m, case.ldb, R, Q[j], ms[j], ie) for j in range(case.nq)]
    answers = tool_thr(audit_exe, requests)
    assert all(code == RB.RANGE_KEYS_FROM for code, _ in answers)
    thr = np.array([t for _, t in answers], dtype=np.float32).reshape(len(case.metrics), 2, case.nq)
    for i, m in enumerate(case.metrics):
        case.thr[m] = [thr[i, 0], thr[i, 1]]
    blocks = run_file(audit_exe, [case], tmp_path)[0]
    for m in case.metrics:
        b = blocks[m]
        assert b["R"] == R and b["Q"].tolist() == Q
        full, half = b["passes"]
        RB.guards_clean(full, ("cnt_guard", "cand_guard"))
        RB.guards_clean(half, ("cnt_guard", "cand_guard"))
        for j, p in enumerate(planted):
            ctx = (case.name, RB.METRIC_NAME[m], j)
            cnt = int(full["cnt"][j])
            assert cnt <= case.cap
            at = np.nonzero(full["pos"][j][:cnt] == p)[0]
            assert len(at) == 1, (ctx, "the planted row is not a candidate under IN_EXTRA_MFMA")
            assert int(half["cnt"][j]) <= case.cap
            assert p not in half["pos"][j][:int(half["cnt"][j])].tolist(), (ctx, "the half-slack threshold still finds the planted row")
            key, bk, ex = float(full["key"][j][at[0]]), float(full["b_key"][j][at[0]]), float(b["exact"][j][p])
            assert ex == case.min_scores[m][j] and ex <= bk, (ctx, "certificate", ex, bk)
            share = RB.slack_share(m, ex, key, bk, case.ldb, R, Q[j])
            SHARE[(m, case.ldb)] = max(SHARE.get((m, case.ldb), 0.0), share)
            COUNTS["planted pairs"] += 1
    assert COUNTS["planted pairs"] % (3 * RB.EDGE_VARIANTS) == 0


# ---- 4. ring and capacity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", RB.RING_DIMS)
def test_ring_segment_filled_exactly_and_by_one_block_too_many(audit_exe, dim, tmp_path):
    seg = RB.rs_seg(RB.mfma_ldb(dim))
    fit, over = RB.ring_case(dim, seg // 32), RB.ring_case(dim, seg // 32 + 1)
    assert fit.note["per_block"] == seg and over.note["per_block"] == seg + 32
    outs = run_file(audit_exe, [fit, over], tmp_path)
    judged = RB.judge_ring(fit, outs[0], fit.note["per_block"]) + RB.judge_ring(over, outs[1], over.note["per_block"])
    assert judged == 2 * 3 * fit.nq
    COUNTS["ring queries"] += judged


@pytest.mark.parametrize("dim", RB.RING_DIMS)
def test_ring_entries_carried_over_a_block(audit_exe, dim, tmp_path):
    seg = RB.rs_seg(RB.mfma_ldb(dim))
    fit, over = RB.carry_case(dim, 2), RB.carry_case(dim, 3)
    assert fit.note["second_block_total"] == seg and over.note["second_block_total"] == seg + 32
    outs = run_file(audit_exe, [fit, over], tmp_path)
    judged = RB.judge_ring(fit, outs[0], seg) + RB.judge_ring(over, outs[1], seg + 32)
    assert judged == 2 * 3 * fit.nq
    COUNTS["ring queries"] += judged


@pytest.mark.parametrize("dim", (128, 768))
def test_small_candidate_buffers(audit_exe, dim, tmp_path):
    base = RB.lattice_case(dim, RB.RING_N, RB.qpc(RB.mfma_ldb(dim)) + 1, 0, 1, cap=RB.CAND_CAP, ranks=RB.RANKS_LIGHT)
    cases = [base, RB.with_cap(base, 1), RB.with_cap(base, 16)]
    outs = run_file(audit_exe, cases, tmp_path)
    judged, exact = RB.judge_lattice(base, outs[0])
    assert exact == judged, "no ring segment overflows in this case"
    for c, o in zip(cases[1:], outs[1:]):
        kinds = set()
        for m in c.metrics:
            for p, p0, t in zip(o[m]["passes"], outs[0][m]["passes"], c.thr[m]):
                # the true sets are the large run's own lists (judged above against the model)
                want = [np.sort(p0["pos"][q][:int(p0["cnt"][q])].astype(np.int64)) for q in range(c.nq)]
                kinds |= {len(w) > c.cap for w in want if len(w)}
                judged += RB.judge_pass(c, m, o[m], p, want, c.note[m])
        assert kinds == {True, False}, "the case must hold queries that fit and queries that do not"
    assert judged == 3 * 3 * 2 * base.nq
    COUNTS["ring queries"] += judged


def test_mixed_gaussian_case_is_right_or_marked(audit_exe, tmp_path):
    """One workgroup per chunk.  Chunk 0 cuts at ranks 5 .. 900 (its waves' segments overflow), chunk 1 at ranks 1 .. 40
    (they do not), chunk 2 is one query at rank 900.  Every query is exactly the host model's set or marked; none is
    silently short, and the chunks the ring held are not marked."""
    ranks = tuple((5, 40, 300, 900)[q % 4] for q in range(128)) + tuple((1, 5, 40)[q % 3] for q in range(128)) + (900,)
    case = RB.rounded_case("gauss", 384, n=RB.RING_N, nq=257, ranks=ranks, cap=RB.CAND_CAP, name="mixed-gauss-d384")
    blocks = run_file(audit_exe, [case], tmp_path)[0]
    judged, marked = RB.judge_rounded(case, blocks, marked_allowed=True)
    assert judged == 3 * case.nq
    for m in case.metrics:
        over = blocks[m]["passes"][0]["cnt"][:case.nq] > case.cap
        assert over[:128].all() and not over[128:].any(), (RB.METRIC_NAME[m], "marks", np.nonzero(over)[0])
    COUNTS["ring queries"] += judged
    COUNTS["of them marked in the mixed case"] += marked


# ---- 5. the tail ---------------------------------------------------------------------------------------------------------------
def judge_tails(exe, cases, tmp_path):
    outs = run_file(exe, cases, tmp_path)
    judged = 0
    for c, o in zip(cases, outs):
        m = c.metrics[0]
        model = RB.tail_model(oracle.calculate, m, c.rows, c.queries, c.cand_pos[m], c.cnt[m], c.cap, c.min_scores[m], c.emit_cap)
        judged += RB.judge_tail(c, m, o[m]["tail"], model)
    assert judged == sum(c.nq for c in cases)
    COUNTS["tail queries"] += judged
    return outs


@pytest.mark.parametrize("dim", RB.TAIL_DIMS)
def test_tail_at_every_candidate_count_and_width(audit_exe, dim, tmp_path):
    judge_tails(audit_exe, RB.tail_cnt_cases(dim), tmp_path)


@pytest.mark.parametrize("metric", RB.ALL4, ids=[RB.METRIC_NAME[m] for m in RB.ALL4])
def test_tail_survivor_counts_around_the_segment(audit_exe, metric, tmp_path):
    outs = judge_tails(audit_exe, [RB.tail_total_case(oracle.calculate, metric)], tmp_path)
    ctr = outs[0][metric]["tail"]["ctr"]
    assert ctr[:, RB.CTR_TOTAL].tolist() == list(RB.TAIL_TOTALS)
    assert ctr[:, RB.CTR_WANT].tolist() == [t if t <= RB.RBATCH_SEG else 0 for t in RB.TAIL_TOTALS]


def test_tail_emit_capacities(audit_exe, tmp_path):
    totals = (0, 1, 2, 3, 40, 41)
    cases = [RB.tail_total_case(oracle.calculate, RB.ALL4[i % 4], emit_cap=e, totals=totals)
             for i, e in enumerate((0, 1, 39, 40, RB.RBATCH_SEG))]
    judge_tails(audit_exe, cases, tmp_path)


@pytest.mark.parametrize("nq", RB.TAIL_NQS)
def test_tail_packs_the_answers_of_many_queries(audit_exe, nq, tmp_path):
    judge_tails(audit_exe, [RB.tail_nq_case(oracle.calculate, RB.ALL4[RB.TAIL_NQS.index(nq) % 4], nq)], tmp_path)


def test_tail_cut_ties_duplicates_and_nan(audit_exe, tmp_path):
    cases = [RB.tail_cut_case(oracle.calculate, m) for m in RB.ALL4] + [RB.tail_tie_case(m) for m in RB.ALL4]
    cases += [RB.tail_nan_case(m) for m in RB.ALL4]
    outs = judge_tails(audit_exe, cases, tmp_path)
    for c, o in zip(cases, outs):
        ctr = o[c.metrics[0]]["tail"]["ctr"]
        if "nan" in c.name:
            assert ctr[:, RB.CTR_NAN].tolist() == [0, 1, 0] and ctr[:, RB.CTR_WANT].tolist() == [16, 0, 16], c.name
            assert ctr[:, RB.CTR_OFF].tolist() == [0, 16, 16], c.name
        if "cut" in c.name:
            assert ctr[:, RB.CTR_TOTAL].tolist()[2:] == [c.cap, 0] and ctr[0, 0] > ctr[1, 0] > 0, (c.name, ctr[:, 0])


# ---- 6. chain --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", RB.CHAIN_DIMS)
def test_pass_and_tail_chained_answer_like_the_oracle(audit_exe, dim, tmp_path):
    orcs = {}

    def rank(metric, rows, q):
        if "o" not in orcs:
            orcs["o"] = oracle.FlatOracle(rows.shape[1], np.arange(len(rows), dtype=np.uint64), rows)
        ids, scores = orcs["o"].search(q, len(rows), metric)
        return ids.astype(np.int64), scores

    case = RB.chain_case(rank, dim)
    answered, handed = RB.judge_chain(case, run_file(audit_exe, [case], tmp_path)[0])
    assert answered + handed == 3 * case.nq
    assert handed >= 3 and answered >= 3 * case.nq // 2, (answered, handed)  # -inf is handed back; the audit is not vacuous
    print(f"\nchain d{dim}: {answered} queries answered on the device, {handed} handed back")
    COUNTS["chain queries"] += answered + handed
