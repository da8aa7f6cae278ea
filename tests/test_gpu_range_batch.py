"""Batched range search (vl_index_search_range_batch): row i of the answer is exactly the single range search of query i
on the same index state.  Every check compares against the oracle's full ranking cut at the threshold in Python (as
tests/test_gpu_range_search.py builds it) AND against the single search_range call on the same handle."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, EUC, MAN, DOT = 0, 1, 2, 3
METRICS = (COS, EUC, MAN, DOT)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def V():
    import vectorlite_amd as V
    n_dev, _ = V.runtime_info()
    assert n_dev > 0, "GPU tests need a HIP device"
    return V


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O
    return O


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64).tolist()


def random_ids(rng, n):
    base = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(rng.integers(1 << 20))) % np.uint64(1 << 40)
    return rng.permutation(base)


def expected(rank, min_score):
    ri, rs = rank
    ok = rs >= min_score  # the IEEE comparison; the ranking is score-descending, so the passing rows are a prefix
    m = int(ok.sum())
    assert bool(ok[:m].all())
    return ri[:m], rs[:m]


def build(V, O, dim, ids, rows):
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    return idx, O.FlatOracle(dim, ids, rows)


def check_batch(idx, ref, queries, min_score, metric, filt=None, limit=None, tag=None, single=True, ranks=None):
    """One batch call against the oracle (and the single call) for every query; returns (totals, routes)."""
    nq = len(queries)
    ms = np.broadcast_to(np.asarray(min_score, dtype=np.float64), (nq,))
    ids_l, scores_l, totals = idx.search_range_batch_arrays(queries, min_score, metric, filter=filt, limit=limit)
    routes = idx.last_range_batch()
    assert len(ids_l) == nq and len(scores_l) == nq and len(totals) == nq
    # the counts describe the last call of the C entry point: with limit=None the wrapper asks the queries with more than 64
    # qualifying rows a second time, as a batch of their own
    over = int((np.asarray(totals) > 64).sum()) if limit is None else 0
    assert routes["mfma_queries"] + routes["single_queries"] + routes["exact_queries"] == (over or nq), (tag, routes)
    for i in range(nq):
        rank = ranks[i] if ranks is not None else ref.search(queries[i], len(ref), metric)
        ei, es = expected(rank, float(ms[i]))
        want = ei.size if limit is None else min(ei.size, limit)
        assert int(totals[i]) == ei.size, (tag, metric, i, float(ms[i]), int(totals[i]), ei.size)
        assert ids_l[i].tolist() == ei[:want].tolist(), (tag, metric, i, float(ms[i]))
        assert bits(scores_l[i]) == bits(es[:want]), (tag, metric, i, float(ms[i]))
        if single:
            si, ss, st = idx.search_range_arrays(queries[i], float(ms[i]), metric, filter=filt, limit=limit)
            assert st == int(totals[i]) and si.tolist() == ids_l[i].tolist() and bits(ss) == bits(scores_l[i]), (tag, metric, i)
    return totals, routes


def mfma_route(dim, metric, nq):
    return metric != MAN and dim <= 768 and nq >= 2


# ---- 1. parity -----------------------------------------------------------------------------------
# 128 / 384 / 768: row lengths with an MFMA shape; 100: padded to 128; 1000: no shape (the loop route)
@pytest.mark.parametrize("dim", [128, 384, 768, 100, 1000])
@pytest.mark.parametrize("metric", METRICS)
def test_parity_on_and_between_scores(V, O, dim, metric):
    rng = np.random.default_rng(1000 * metric + dim)
    n = 3000
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    if metric == COS:
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    idx, ref = build(V, O, dim, ids, rows)
    for nq in (1, 2, 3, 129):
        queries = rng.standard_normal((nq, dim))
        ranks = [ref.search(q, n, metric) for q in queries]
        at = np.array([ranks[i][1][(0, 3, 9, 20)[i % 4]] for i in range(nq)])
        for name, ms in (("on", at), ("above", np.nextafter(at, np.inf)), ("below", np.nextafter(at, -np.inf))):
            _, routes = check_batch(idx, ref, queries, ms, metric, tag=(dim, nq, name), ranks=ranks)
            if mfma_route(dim, metric, nq):  # a few rows per query: nothing overflows, the whole batch is the MFMA pass
                assert routes["mfma_queries"] == nq, (dim, metric, nq, name, routes)
            else:
                assert routes["mfma_queries"] == 0, (dim, metric, nq, name, routes)
        # a scalar threshold for the whole batch, low enough that a tenth of the rows qualify for some queries (whichever
        # route answers: ring segments may overflow here)
        scalar = float(np.median([r[1][150] for r in ranks]))
        check_batch(idx, ref, queries, scalar, metric, tag=(dim, nq, "scalar"), ranks=ranks)


def test_more_than_one_launch_sequence(V, O):
    rng = np.random.default_rng(77)
    n, dim, nq = 2000, 384, 2500
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    idx, ref = build(V, O, dim, ids, rows)
    queries = rng.standard_normal((nq, dim))
    ranks = [ref.search(q, 64, COS) for q in queries]  # thresholds within the top 12: the top 64 holds every qualifying row
    ms = np.array([ranks[i][1][i % 12] for i in range(nq)])
    ids_l, scores_l, totals = idx.search_range_batch_arrays(queries, ms, COS)
    routes = idx.last_range_batch()
    assert routes["mfma_queries"] == nq, routes
    for i in range(nq):
        ei, es = expected(ranks[i], float(ms[i]))
        assert ei.size < 64 and int(totals[i]) == ei.size and ids_l[i].tolist() == ei.tolist() and bits(scores_l[i]) == bits(es), i
    for i in range(nq):  # row i == the single call, for every query
        si, ss, st = idx.search_range_arrays(queries[i], float(ms[i]), COS)
        assert st == int(totals[i]) and si.tolist() == ids_l[i].tolist() and bits(ss) == bits(scores_l[i])


# ---- 2. ties and order ---------------------------------------------------------------------------
def test_duplicate_blocks_across_block_wave_and_workgroup_boundaries(V, O):
    rng = np.random.default_rng(3)
    n, dim = 20_000, 384
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    # runs of identical rows over the boundaries of a 32-row block, a 64-row tile, a workgroup's 8 x 32 rows, and further in
    blocks = [(28, 37), (60, 70), (250, 262), (2040, 2060), (8190, 8200), (19_990, 20_000)]
    for a, b in blocks:
        rows[a:b] = rows[a]
    idx, ref = build(V, O, dim, ids, rows)
    queries = np.stack([rows[a] + 0.01 * rng.standard_normal(dim) for a, _ in blocks] * 2)
    for metric in (COS, EUC, DOT, MAN):
        ranks = [ref.search(q, n, metric) for q in queries]
        ms = []
        for i, (a, b) in enumerate(blocks * 2):
            ri, rs = ranks[i]
            at = int(np.nonzero(ri == ids[a])[0][0])      # the block's first row: its copies follow it in insertion order
            assert ri[at:at + (b - a)].tolist() == ids[a:b].tolist()
            ms.append(rs[at])                             # the threshold ties with every copy: all of them are in
        _, routes = check_batch(idx, ref, queries, np.array(ms), metric, tag="dups", ranks=ranks)
        if metric != MAN:
            assert routes["mfma_queries"] > 0, routes


# ---- 3. capacity ---------------------------------------------------------------------------------
def test_capacity_count_only_infinities_zero_query_empty(V, O):
    rng = np.random.default_rng(4)
    n, dim = 500, 128
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    idx, ref = build(V, O, dim, ids, rows)
    queries = rng.standard_normal((6, dim))
    queries[4] = 0.0  # a zero query: every cosine score is 0.0
    for metric in METRICS:
        ranks = [ref.search(q, n, metric) for q in queries]
        ms = np.array([ranks[0][1][40], ranks[1][1][2], -np.inf, np.inf, 0.0, ranks[5][1][0]])
        for limit in (None, 5, 1, 0):  # a prefix; total always right; 0 = count only (NULL outputs)
            totals, routes = check_batch(idx, ref, queries, ms, metric, limit=limit, tag=("cap", limit), ranks=ranks)
            assert int(totals[2]) == n and int(totals[3]) == 0
        if metric == COS:
            assert int(totals[4]) == n  # 0.0 >= 0.0 for every row
            assert routes["mfma_queries"] == 4 and routes["single_queries"] == 2, routes  # -inf and the zero query are peeled off
    empty = V.FlatIndex(dim)
    ids_l, scores_l, totals = empty.search_range_batch_arrays(queries, 0.5, COS)
    assert [x.size for x in ids_l] == [0] * 6 and totals.tolist() == [0] * 6
    ids_l, scores_l, totals = idx.search_range_batch_arrays(np.zeros((0, dim)), 0.5, COS)  # nq = 0
    assert ids_l == [] and scores_l == [] and totals.size == 0
    r = idx.last_range_batch()
    assert r["mfma_queries"] + r["single_queries"] + r["exact_queries"] == 0
    rc = idx._L.vl_index_search_range_batch(idx._h, 0, None, 0, dim, None, COS, 0, None, None, None, None)
    assert rc == 0  # VL_OK, nothing written (nothing to write to)


# ---- 4. routing ----------------------------------------------------------------------------------
def test_route_whole_batch_on_the_mfma_pass(V, O):
    """The issue's condition: 200 000 random unit rows, dim 384, cosine, 256 queries, each threshold at that query's 20th best
    oracle score -> no query leaves the MFMA route.  (Cosine scores have sigma ~ 0.051, the bf16 slack is under 0.009: tens
    of candidates per query against a buffer of 4096.)"""
    n, dim, nq = 200_000, 384, 256
    rows = np.random.default_rng(1234).standard_normal((n, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    queries = np.random.default_rng(4321).standard_normal((nq, dim))
    queries /= np.linalg.norm(queries, axis=1, keepdims=True)
    ids = np.arange(n, dtype=np.uint64) + np.uint64(11)
    idx, ref = build(V, O, dim, ids, rows)
    ranks = [ref.search(q, 64, COS) for q in queries]
    ms = np.array([r[1][19] for r in ranks])
    ids_l, scores_l, totals = idx.search_range_batch_arrays(queries, ms, COS)
    routes = idx.last_range_batch()
    print("largest candidate count of a query:", routes["max_candidates"], "routes:", routes)
    assert routes["single_queries"] == 0 and routes["exact_queries"] == 0 and routes["mfma_queries"] == nq, routes
    for i in range(nq):
        ei, es = expected(ranks[i], float(ms[i]))
        assert 20 <= ei.size < 64 and int(totals[i]) == ei.size
        assert ids_l[i].tolist() == ei.tolist() and bits(scores_l[i]) == bits(es)
    for i in range(nq):  # row i == the single call, for every query
        si, ss, st = idx.search_range_arrays(queries[i], float(ms[i]), COS)
        assert st == int(totals[i]) and si.tolist() == ids_l[i].tolist() and bits(ss) == bits(scores_l[i])


_OVERFLOW_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import vectorlite_amd as V
from oracle import oracle as O
rng = np.random.default_rng(6)
n, dim, nq = 20_000, 384, 40
ids = np.arange(n, dtype=np.uint64) + np.uint64(5)
rows = rng.standard_normal((n, dim))
idx = V.FlatIndex(dim)
idx.add_rows(ids, rows, validate=False)
ref = O.FlatOracle(dim, ids, rows)
queries = rng.standard_normal((nq, dim))
for metric in (0, 1, 3):
    ranks = [ref.search(q, n, metric) for q in queries]
    # even queries: 3 rows qualify (a handful of candidates); odd queries: 400 rows qualify (far more than 16 candidates)
    ms = np.array([ranks[i][1][2 if i % 2 == 0 else 399] for i in range(nq)])
    ids_l, scores_l, totals = idx.search_range_batch_arrays(queries, ms, metric, limit=512)  # one call: every total fits
    r = idx.last_range_batch()
    assert r["mfma_queries"] + r["single_queries"] + r["exact_queries"] == nq, r
    assert r["single_queries"] + r["exact_queries"] >= nq // 2, (metric, r)   # every odd query overflowed 16 entries
    assert r["max_candidates"] <= 16, r
    for i in range(nq):
        ri, rs = ranks[i]
        m = int((rs >= ms[i]).sum())
        assert int(totals[i]) == m and ids_l[i].tolist() == ri[:m].tolist(), (metric, i, int(totals[i]), m)
        assert scores_l[i].view(np.uint64).tolist() == rs[:m].view(np.uint64).tolist(), (metric, i)
    print("routes", metric, r)
print("overflow-ok")
"""


def test_candidate_overflow_is_answered_by_the_single_call(V, O, tmp_path):
    """With the per-query candidate buffers lowered to 16 entries (a fresh process: the knob is the process's environment),
    queries with more candidates leave the MFMA route, are counted as single / exact queries and are still exact."""
    script = tmp_path / "range_batch_overflow_child.py"
    script.write_text(_OVERFLOW_CHILD)
    env = dict(os.environ, VL_RANGE_BATCH_CAND_CAP="16")
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "overflow-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    print(r.stdout)


def test_more_qualifying_rows_than_the_segmented_rank_holds(V, O):
    rng = np.random.default_rng(8)
    n, dim = 40_000, 128
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    idx, ref = build(V, O, dim, ids, rows)
    queries = rng.standard_normal((4, dim))
    ranks = [ref.search(q, n, DOT) for q in queries]
    ms = np.array([ranks[0][1][5], ranks[1][1][2999], ranks[2][1][1500], ranks[3][1][0]])  # 3000 > 2048 survivors for query 1
    _, routes = check_batch(idx, ref, queries, ms, DOT, tag="seg", ranks=ranks)
    assert routes["single_queries"] + routes["exact_queries"] >= 1, routes
    check_batch(idx, ref, queries, ms, DOT, limit=7, tag="seg-limit", ranks=ranks)


# ---- 5. mixed batches ----------------------------------------------------------------------------
def test_mixed_domains_and_forced_path(V, O):
    rng = np.random.default_rng(9)
    n, dim = 5000, 128
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    idx, ref = build(V, O, dim, ids, rows)
    queries = rng.standard_normal((8, dim))
    queries[2, 3] = 2.0 ** 45  # outside the fast-path domain: answered on the exact route
    queries[6, 0] = 2.0 ** 41
    for metric in METRICS:
        ranks = [ref.search(q, n, metric) for q in queries]
        ms = np.array([r[1][10] for r in ranks])
        _, routes = check_batch(idx, ref, queries, ms, metric, tag="mixed", ranks=ranks)
        if metric != MAN:
            assert routes["mfma_queries"] == 6 and routes["exact_queries"] == 2, routes
        else:
            assert routes["mfma_queries"] == 0 and routes["exact_queries"] == 2, routes
    idx.force_path(V.PATH_EXACT_SORT)
    try:
        ranks = [ref.search(q, n, COS) for q in queries]
        _, routes = check_batch(idx, ref, queries, np.array([r[1][10] for r in ranks]), COS, tag="forced", ranks=ranks)
        assert routes["exact_queries"] == 8, routes
    finally:
        idx.force_path(0)
    big = rows.copy()
    big[99, 5] = 2.0 ** 41  # an out-of-domain row: the whole batch leaves the fast path
    idx2, ref2 = build(V, O, dim, ids, big)
    good = rng.standard_normal((5, dim))
    ranks = [ref2.search(q, n, COS) for q in good]
    _, routes = check_batch(idx2, ref2, good, np.array([r[1][10] for r in ranks]), COS, tag="big-row", ranks=ranks)
    assert routes["mfma_queries"] == 0 and routes["exact_queries"] == 5, routes


def test_nan_status_is_the_lowest_failing_querys(V, O):
    rng = np.random.default_rng(10)
    n, dim = 1000, 128
    ids = np.arange(n, dtype=np.uint64)
    rows = rng.standard_normal((n, dim))
    clean, _ = build(V, O, dim, ids, rows)
    queries = rng.standard_normal((4, dim))
    with pytest.raises(V.IndexOpError, match="NaN"):  # a NaN threshold, as the single call reports it
        clean.search_range_batch_arrays(queries, np.array([0.5, 0.5, np.nan, 0.5]), COS)
    rows[500, 3] = np.nan
    idx, ref = build(V, O, dim, ids, rows)
    for metric in METRICS:
        with pytest.raises(O.OracleError):
            ref.search(queries[0], n, metric)
        with pytest.raises(V.NaNScore):
            idx.search_range_arrays(queries[0], 0.5, metric)
        with pytest.raises(V.NaNScore):
            idx.search_range_batch_arrays(queries, 0.5, metric)
        with pytest.raises(V.NaNScore):  # query 0 fails with the NaN score before query 1's NaN threshold is looked at
            idx.search_range_batch_arrays(queries, np.array([0.5, np.nan, 0.5, 0.5]), metric)
        with pytest.raises(V.IndexOpError, match="NaN"):  # query 0's NaN threshold comes first
            idx.search_range_batch_arrays(queries, np.array([np.nan, 0.5, 0.5, 0.5]), metric)
    outside = [int(x) for x in ids if x != 500]  # a subset without the NaN row answers
    sub = O.FlatOracle(dim, ids[ids != 500], rows[ids != 500])
    ranks = [sub.search(q, n - 1, COS) for q in queries]
    check_batch(idx, sub, queries, np.array([r[1][5] for r in ranks]), COS, filt=outside, tag="nan-subset", ranks=ranks)
    with pytest.raises(V.NaNScore):
        idx.search_range_batch_arrays(queries, 0.5, COS, filter=[1, 2, 500, 7])


# ---- 6. filters ----------------------------------------------------------------------------------
def test_filter_gives_the_filtered_single_result_and_follows_mutations(V, O):
    rng = np.random.default_rng(11)
    n, dim = 5000, 128
    ids = np.arange(n, dtype=np.uint64) * np.uint64(2)
    rows = rng.standard_normal((n, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    keep = [int(x) for x in ids[1::3]] + [20_001, 20_003]
    queries = rng.standard_normal((5, dim))
    f = idx.make_filter(keep)

    def agree():
        eids, evals = idx.export()
        sel = np.isin(eids, np.asarray(keep, dtype=np.uint64))
        ref = O.FlatOracle(dim, eids[sel], evals[sel])
        for metric in (COS, MAN):
            ranks = [ref.search(q, len(ref), metric) for q in queries]
            ms = np.array([ranks[i][1][(0, 30, len(ref) - 1, 7, 100)[i]] for i in range(5)])
            _, routes = check_batch(idx, ref, queries, ms, metric, filt=f, tag="filter", ranks=ranks)
            assert routes["mfma_queries"] == 0, routes  # filtered batches are a loop over the single call

    agree()
    idx.add(V.Vector(id=20_001, values=list(queries[0] * 1.5)))
    agree()
    idx.add_rows(np.array([20_003, 20_007], dtype=np.uint64), rng.standard_normal((2, dim)))
    agree()
    for d in (int(ids[0]), int(ids[4]), 20_003):
        idx.delete(d)
        agree()
    f.close()
    with idx.make_filter([1 << 50]) as e:  # an empty subset
        ids_l, _, totals = idx.search_range_batch_arrays(queries, -np.inf, COS, filter=e)
        assert totals.tolist() == [0] * 5 and all(x.size == 0 for x in ids_l)


# ---- 7. concurrency ------------------------------------------------------------------------------
def test_concurrent_batches_and_topk_searches_while_a_writer_adds(V, O):
    rng = np.random.default_rng(13)
    n, dim, nq = 30_000, 128, 6
    ids = np.arange(n, dtype=np.uint64)
    rows = rng.standard_normal((n, dim))
    queries = rng.standard_normal((nq, dim))
    extra = [(np.arange(n, n + 500, dtype=np.uint64), np.vstack([queries * 2.0, rng.standard_normal((500 - nq, dim))])),
             (np.arange(n + 500, n + 900, dtype=np.uint64), np.vstack([queries * 3.0, rng.standard_normal((400 - nq, dim))]))]
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    ref = O.FlatOracle(dim, ids, rows)
    ts = np.array([ref.search(q, n, COS)[1][49] for q in queries])  # fixed thresholds: 50 rows qualify at first, then more
    states = []
    for step in [None] + extra:
        if step is not None:
            ref.extend(*step)
        batch, topk = [], None
        for i, q in enumerate(queries):
            ri, rs = ref.search(q, len(ref), COS)
            ei, es = expected((ri, rs), float(ts[i]))
            batch.append((ei.tolist(), bits(es)))
            if i == 0:
                topk = (ri[:10].tolist(), bits(rs[:10]))
        states.append((batch, topk))
    answers = [[] for _ in range(6)]
    stop = threading.Event()

    def reader(i):
        while True:
            last = stop.is_set()
            if i % 2 == 0:
                il, sl, totals = idx.search_range_batch_arrays(queries, ts, COS)
                assert [int(t) for t in totals] == [x.size for x in il]
                answers[i].append((0, [(a.tolist(), bits(b)) for a, b in zip(il, sl)]))
            else:
                gi, gs = idx.search_arrays(queries[0], 10, COS)
                answers[i].append((1, (gi.tolist(), bits(gs))))
            if last:
                return

    th = [threading.Thread(target=reader, args=(i,)) for i in range(6)]
    for x in th:
        x.start()
    for step in extra:
        idx.add_rows(*step)
    stop.set()
    for x in th:
        x.join()
    for i in range(6):
        assert answers[i]
        for kind, a in answers[i]:
            assert any(a == s[kind] for s in states)  # the WHOLE batch equals the oracle at ONE index state
        assert answers[i][-1][1] == states[2][answers[i][-1][0]]  # the pass after the writer finished sees every row


# ---- 8. errors -----------------------------------------------------------------------------------
def test_errors(V):
    rng = np.random.default_rng(14)
    idx = V.FlatIndex(8)
    idx.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    qs = np.ones((3, 8))
    with pytest.raises(V.DimensionMismatch):
        idx.search_range_batch_arrays(np.zeros((3, 7)), 0.5, COS)
    with pytest.raises(V.IndexOpError, match="metric"):
        idx.search_range_batch_arrays(qs, 0.5, 7)
    with pytest.raises(V.IndexOpError, match="NaN"):
        idx.search_range_batch_arrays(qs, float("nan"), COS)
    f = idx.make_filter([1, 2])
    tok = f.token
    f.close()
    n_out, tot = np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64)
    out_i, out_s = np.zeros(12, dtype=np.uint64), np.zeros(12)
    ms = np.full(3, 0.5)
    rc = idx._L.vl_index_search_range_batch(idx._h, tok, qs.ctypes.data, 3, 8, ms.ctypes.data, COS, 4, out_i.ctypes.data,
                                            out_s.ctypes.data, n_out.ctypes.data, tot.ctypes.data)
    assert rc == 8  # VL_ERR_INVALID_ARG: unknown filter
    empty = V.FlatIndex(8)
    assert empty.search_range_batch_arrays(np.zeros((2, 3)), 0.5, COS)[2].tolist() == [0, 0]  # an empty index checks no dimension
    with pytest.raises(V.IndexOpError, match="NaN"):
        empty.search_range_batch_arrays(np.zeros((2, 3)), np.array([0.5, np.nan]), COS)
    hn = V.HNSWIndex(8)
    hn.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        hn.search_range_batch_arrays(qs, 0.5, COS)
    mi = V.MultiFlatIndex(8, [0, 0])
    mi.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        mi.search_range_batch_arrays(qs, 0.5, COS)
    a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    assert idx._L.vl_index_last_range_batch(mi._h, C.byref(a), C.byref(b), C.byref(c)) == 8
    res = idx.search_range_batch(qs, -np.inf, V.SimilarityMetric.Cosine)
    assert len(res) == 3 and all(len(r) == 10 for r in res)
    assert [x.id for x in res[0]] == idx.search_range_arrays(qs[0], -np.inf, COS)[0].tolist()
