"""The host model of tests/_range_batch_cases.py against FlatOracle, and the preconditions of its constructed cases.

tests/test_gpu_range_batch_audit.py judges the batched range search's tail with tail_model; here the model is shown right
first, without a GPU: handed every row of a small index as a candidate it must answer like FlatOracle's full ranking cut
at the threshold, ties and signed zeros included.  The constructions the pass is judged with are checked as well: exact
lattice sums, thresholds in gaps no allowance reaches, planted pairs that lose what they are meant to lose, ring cases that
fill a segment to the entry.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _range_batch_cases as RB  # noqa: E402
from oracle import oracle  # noqa: E402

NAMES = [RB.METRIC_NAME[m] for m in RB.ALL4]


@pytest.mark.parametrize("metric", RB.ALL4, ids=NAMES)
def test_tail_model_answers_like_flat_oracle(metric):
    rng = np.random.default_rng([1, metric])
    n, dim = 300, 3
    rows = RB.mixed_rows(rng, n, dim)   # 7^3 possible rows for 300: equal rows and equal scores everywhere
    rows[200:230] = rows[17]            # and equal rows: the lower position leaves first
    orc = oracle.FlatOracle(dim, np.arange(n, dtype=np.uint64), rows)
    queries = rng.integers(-3, 4, size=(6, dim)).astype(np.float64)
    queries[~queries.any(axis=1), 0] = 1.0
    cand = np.stack([rng.permutation(n) for _ in queries])
    mins, ranks = [], []
    for i, q in enumerate(queries):
        ids, sc = orc.search(q, n, metric)
        ranks.append((ids, sc))
        on = float(sc[(0, 10, 150, n - 1)[i % 4]])
        mins.append((on, float(np.nextafter(on, np.inf)), -np.inf, np.inf, on, on)[i])
    for emit_cap in (0, 7, RB.RBATCH_SEG):
        model = RB.tail_model(oracle.calculate, metric, rows, queries, cand, [n] * 6, n, mins, emit_cap)
        off = 0
        for (ids, sc), ms, r in zip(ranks, mins, model):
            keep = sc >= ms
            m = int(keep.sum())
            assert r["total"] == m and r["nan"] == 0 and r["want"] == min(m, emit_cap) and r["off"] == off
            assert r["out_pos"].tolist() == ids[:r["want"]].tolist()
            assert r["out_bits"].tolist() == RB.bits64(sc[:r["want"]]).tolist()
            off += r["want"]
    assert any(len(np.unique(sc)) < n // 2 for _, sc in ranks), "the index must tie"


def test_tail_model_rules():
    scores = {0: 0.0, 1: -0.0, 2: 1.0, 3: -0.0, 4: 0.0, 5: float("nan"), 6: -1.0}
    rows = np.arange(7, dtype=np.float64)[:, None]

    def calc(metric, row, q):
        return scores[int(row[0])]

    q = np.zeros((4, 1))
    cand = [np.array([4, 3, 2, 1, 0, 3]), np.array([6, 5, 2]), np.array([0, 1, 2, 9]), np.array([2, 2, 2])]
    model = RB.tail_model(calc, RB.DOT, rows, q, cand, [6, 3, 9, 3], 8, [-0.0, -5.0, 0.0, 0.5], 5)
    a, b, c, d = model
    # +0.0 and -0.0 tie, leave by position with their own bits; a position listed twice leaves twice
    assert a["out_pos"].tolist() == [2, 0, 1, 3, 3] and a["total"] == 6 and a["want"] == 5
    assert a["out_bits"].tolist() == RB.bits64([1.0, 0.0, -0.0, -0.0, -0.0]).tolist()
    # a NaN: the flag, no answer, and the next query starts where this one did
    assert (b["nan"], b["want"], b["total"]) == (1, 0, 2) and b["off"] == 5 and d["off"] == 5
    # a counter above the capacity: nothing of the query is looked at
    assert (c["total"], c["want"], c["nan"]) == (0, 0, 0)
    assert d["out_pos"].tolist() == [2, 2, 2]
    # more survivors than the segment holds: counted, not answered
    many = RB.tail_model(calc, RB.DOT, rows, q[:1], [np.full(RB.RBATCH_SEG + 1, 2)], [RB.RBATCH_SEG + 1], RB.CAND_CAP, [0.0], 9)
    assert many[0]["total"] == RB.RBATCH_SEG + 1 and many[0]["want"] == 0


def test_tail_cases_hold_what_they_are_there_for():
    tie = RB.tail_tie_case(RB.DOT)
    sc = [oracle.calculate(RB.DOT, tie.rows[p], tie.queries[1]) for p in (90, 94)]
    assert RB.bits64(sc).tolist() == RB.bits64([0.0, -0.0]).tolist(), "rows of +0.0 / -0.0 must score +0.0 / -0.0"
    for m in RB.ALL4:
        nan = RB.tail_nan_case(m)
        assert np.isnan(oracle.calculate(m, nan.rows[7], nan.queries[1]))
        cut = RB.tail_cut_case(oracle.calculate, m)
        model = RB.tail_model(oracle.calculate, m, cut.rows, cut.queries, cut.cand_pos[m], cut.cnt[m], cut.cap, cut.min_scores[m], 2048)
        assert model[0]["total"] > model[1]["total"] > 0 and model[2]["total"] == cut.cap and model[3]["total"] == 0
    total = RB.tail_total_case(oracle.calculate, RB.EUC)
    model = RB.tail_model(oracle.calculate, RB.EUC, total.rows, total.queries, total.cand_pos[RB.EUC], total.cnt[RB.EUC], total.cap,
                          total.min_scores[RB.EUC], 2048)
    assert [r["total"] for r in model] == list(RB.TAIL_TOTALS)
    for dim in RB.TAIL_DIMS[:2]:
        cases = RB.tail_cnt_cases(dim)
        assert [c.metrics[0] for c in cases] == list(RB.ALL4)
        assert sorted(cases[0].cnt[RB.COS].tolist()) == sorted(list(RB.TAIL_CNTS) + [130, 131])


def test_lattice_shapes_cover_every_axis():
    for dim in RB.PASS_DIMS:
        ldb = RB.mfma_ldb(dim)
        shapes = RB.lattice_shapes(dim)
        assert {n for n, _, g, _ in shapes if g == 1} == {1024 + r for r in RB.GRID1_TAILS}
        assert {n for n, _, g, _ in shapes if g == 0} == set(RB.SMALL_N)
    for ldb in (128, 256, 384, 512, 768):
        shapes = [s for d in RB.PASS_DIMS if RB.mfma_ldb(d) == ldb for s in RB.lattice_shapes(d)]
        assert {nq for _, nq, _, _ in shapes} == set(RB.nq_list(ldb)), ldb
        one_chunk = {s for _, nq, _, s in shapes if nq <= RB.qpc(ldb)}
        assert one_chunk == {0, 1}, (ldb, "both load forms on a single chunk")
    assert {RB.mfma_ldb(d) for d in RB.PASS_DIMS} == {128, 256, 384, 512, 768}


@pytest.mark.parametrize("dim", (100, 768))
def test_lattice_cases_are_exact_and_fit(dim):
    for shape in RB.lattice_shapes(dim)[::3]:
        c = RB.lattice_case(dim, *shape)  # asserts the exactness of every sum and that no buffer fills
        for m in c.metrics:
            on, above = c.thr[m]
            sets_on, sets_above = RB.sets_at(c.note[m], on), RB.sets_at(c.note[m], above)
            assert all(len(a) < len(b) for a, b, t in zip(sets_above, sets_on, on) if np.isfinite(t)), "the tie is in, then out"
            assert c.expected_info()[1] == -(-c.nq // RB.qpc(c.ldb))


@pytest.mark.parametrize("dim", RB.ROUNDED_DIMS)
def test_rounded_cases_have_their_gaps(dim):
    for fam in RB.ROUNDED_FAMILIES:
        c = RB.rounded_case(fam, dim)  # asserts a gap wider than twice the allowance for every query
        for m in c.metrics:
            kh, tol = c.note[m]
            t = c.thr[m][0].astype(np.float64)
            assert (np.abs(kh - t[:, None]) > 2.0 * tol).all()
            assert 0 < min(len(s) for s in RB.sets_at(kh, t)) and max(len(s) for s in RB.sets_at(kh, t)) <= c.cap


@pytest.mark.parametrize("dim", RB.EDGE_DIMS)
def test_planted_pairs_lose_the_slack(dim):
    c = RB.edge_case(dim)
    norms = np.linalg.norm(c.rows, axis=1)
    assert norms.argmax() in c.note["planted"] and min(norms[c.note["planted"]]) * 1.21 > norms.max() and abs(norms.max() - 1.0) > 0.5
    for m in c.metrics:
        for exact, part in RB.edge_product_and_key(c, m):
            loss = 1.0 - part / exact
            assert RB.EDGE_LOSS <= loss < 1.0 - (1.0 - 2.0 ** -8 / (1.0 + 2.0 ** -8)) ** 2, (dim, m, loss)
            assert loss > RB.IN_EXTRA_BF16_SINGLE * 1.21 + 4.0 * (c.ldb + 4) * RB.U  # the half-slack bound cannot cover it


@pytest.mark.parametrize("dim", RB.RING_DIMS)
def test_ring_cases_fill_the_segment_to_the_entry(dim):
    seg = RB.rs_seg(RB.mfma_ldb(dim))
    assert RB.ring_case(dim, seg // 32).note["per_block"] == seg
    assert RB.carry_case(dim, 2).note["second_block_total"] == seg and RB.carry_case(dim, 3).note["second_block_total"] == seg + 32
    c = RB.ring_case(dim, seg // 32 + 1)
    assert RB.ring_marked(c, c.note["per_block"]).sum() == RB.qpc(c.ldb) and not RB.ring_marked(c, seg).any()
    for m in c.metrics:  # the cold queries of chunk 0 have no candidate, those of chunk 1 have some
        sets = RB.sets_at(c.note[m], c.thr[m][0])
        cold0 = [q for q in range(RB.qpc(c.ldb)) if q not in c.note["hot"]]
        assert all(len(sets[q]) == 0 for q in cold0) and all(len(sets[q]) == c.n for q in c.note["hot"])
        assert sum(len(sets[q]) for q in range(RB.qpc(c.ldb), c.nq)) > 0
