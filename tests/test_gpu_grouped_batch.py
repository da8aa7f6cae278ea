"""Batched grouped search (vl_index_search_grouped_batch).  Row i of a batch is what the single grouped
search returns for query i: checked against the contract restated in Python (tests/test_gpu_grouped_search.py's Case: the
oracle over S, collapsed by a loop) and, row for row, against the loop of single calls on the same handle -- group keys,
ids and score bits with ==.  Every parity case also asserts that the MFMA pass took the batch, and the cases on random rows
that it settled queries itself: parity through hand-backs alone would prove nothing about the pass."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_grouped_search import COS, DOT, EUC, MAN, Case, bits, group_key, make_case, queries_for, random_ids, unit_rows  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(9_000, 128), (12_345, 384), (20_000, 768)]  # just above MFMA_MIN_ROWS = 8192, three kernel strides
SHAPES = ["one_per_group", "eight_per_group", "partial", "clustered"]
MFMA_METRICS = (COS, EUC, DOT)
NQ = 12


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


_CASES = {}


def shared_case(V, O, shape, n, dim):
    """one index, table and query set per (shape, size): the metrics of the parity test share it and its oracle answers"""
    key = (shape, n, dim)
    if key not in _CASES:
        case, rng = make_case(V, O, shape, dim, n, 7 * dim + len(shape))
        _CASES[key] = (case, np.ascontiguousarray(queries_for(case, rng, shape, count=NQ)))
    return _CASES[key]


def check_rows(case, Q, k, metric, got, allowed=None, tag=None):
    keys, ids, scores, cnt = got
    assert keys.shape == ids.shape == scores.shape == (len(Q), k) and cnt.shape == (len(Q),)
    for i, q in enumerate(Q):
        ek, ei, es = case.answer(q, metric, allowed)
        m = int(cnt[i])
        assert m == min(k, len(ek)), (tag, metric, k, i)
        assert keys[i, :m].tolist() == ek[:k], (tag, metric, k, i)
        assert ids[i, :m].tolist() == ei[:k], (tag, metric, k, i)
        assert bits(scores[i, :m]) == es[:k], (tag, metric, k, i)


def equal_to_the_loop(idx, table, Q, k, metric, got, filt=None, tag=None):
    keys, ids, scores, cnt = got
    for i, q in enumerate(Q):
        lk, li, ls = idx.search_grouped_arrays(q, k, metric, groups=table, filter=filt)
        m = int(cnt[i])
        assert m == lk.size, (tag, i)
        assert keys[i, :m].tolist() == lk.tolist() and ids[i, :m].tolist() == li.tolist(), (tag, i)
        assert bits(scores[i, :m]) == bits(ls), (tag, i)


# ---- 1. parity with the restated contract ---------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", MFMA_METRICS)
@pytest.mark.parametrize("n,dim", SIZES)
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_with_the_restated_contract(V, O, shape, n, dim, metric):
    case, Q = shared_case(V, O, shape, n, dim)
    case.idx.set_grouped_batch("on")
    for k in (1, 10, 60):
        got = case.idx.search_grouped_batch_arrays(Q, k, metric, groups=case.table)
        st = case.idx.last_grouped_batch()
        print(f"{shape} {n} x {dim} metric {metric} k {k}: {st}")
        assert st["routed"] == NQ and st["routed"] == st["settled"] + st["handed_back"], st
        assert st["sequences"] == 1
        check_rows(case, Q, k, metric, got, tag=(shape, n, dim))
        if k == 10 and shape in ("one_per_group", "eight_per_group"):
            assert st["settled"] > 0, st  # otherwise the parity above proved nothing about the pass
            assert V.last_path() == V.PATH_FAST
    ungrouped = set(case.ids[~case.has].tolist())
    if ungrouped:
        assert not (set(got[1].ravel().tolist()) & ungrouped)


# ---- 2. row for row the loop of single calls, handed-back queries included ---------------------------------------------------
def test_rows_equal_the_loop_of_single_calls_with_handed_back_queries(V, O):
    rng = np.random.default_rng(31)
    n, dim, k = 10_000, 128, 10
    ids = random_ids(rng, n)
    rows = unit_rows(rng, n, dim)
    g = rng.integers(n // 8, size=n) + 10
    # a 200-row near-duplicate group: it fills a query's whole candidate list, so the prefix holds ONE group
    centre = unit_rows(rng, 1, dim)[0]
    dup = rng.choice(n, 200, replace=False)
    rows[dup] = centre + 1e-4 * rng.standard_normal((200, dim))
    g[dup] = 3
    # eight copies of one row split over two groups: equal scores, the storage order decides -- next to the cut at k = 2
    free = np.setdiff1d(np.arange(n), dup)
    eight = rng.choice(free, 8, replace=False)
    rows[eight] = unit_rows(rng, 1, dim)[0]
    g[eight[::2]] = 4
    g[eight[1::2]] = 5
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    table = idx.make_groups(ids, group_key(g))
    idx.set_grouped_batch("on")
    base = rng.standard_normal((6, dim))
    Q = np.ascontiguousarray(np.vstack([np.zeros(dim), base[0] * 1e200, centre, rows[eight[0]], base]))
    for metric in MFMA_METRICS:
        for kk in (2, k):
            got = idx.search_grouped_batch_arrays(Q, kk, metric, groups=table)
            st = idx.last_grouped_batch()
            print(f"metric {metric} k {kk}: {st}")
            assert st["routed"] == len(Q) and st["routed"] == st["settled"] + st["handed_back"]
            equal_to_the_loop(idx, table, Q, kk, metric, got, tag=(metric, kk))
            if metric == COS and kk == k:
                assert st["handed_back"] >= 3, st  # the zero query, the scaled one, the one aimed at the planted group
                assert st["settled"] > 0, st
    # the copies: both groups come out, each shown by its FIRST copy in storage order
    got = idx.search_grouped_batch_arrays(Q[3:4].repeat(2, axis=0), 2, COS, groups=table)
    first4, first5 = int(ids[np.sort(eight[::2])[0]]), int(ids[np.sort(eight[1::2])[0]])
    assert sorted(got[1][0].tolist()) == sorted([first4, first5])
    assert got[1][0].tolist() == got[1][1].tolist()


# ---- 3. filters ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["include 1 %", "include 30 %", "include 100 %", "exclude 0", "exclude 50", "exclude 5000"])
def test_filters_of_both_kinds(V, O, what):
    n, dim, k = 12_345, 384, 10
    case, Q = shared_case(V, O, "partial", n, dim)
    case.idx.set_grouped_batch("on")
    rng = np.random.default_rng(len(what))
    kind, amount = what.split(" ", 1)
    if kind == "include":
        count = {"1 %": n // 100, "30 %": 3 * n // 10, "100 %": n}[amount]
        chosen = rng.choice(n, count, replace=False)
        allowed = np.zeros(n, dtype=bool)
        allowed[chosen] = True
        f = case.idx.make_filter(case.ids[chosen])
    else:
        chosen = rng.choice(n, int(amount), replace=False)
        allowed = np.ones(n, dtype=bool)
        allowed[chosen] = False
        f = case.idx.make_filter(case.ids[chosen], exclude=True)
    with f:
        for metric in MFMA_METRICS:
            got = case.idx.search_grouped_batch_arrays(Q, k, metric, groups=case.table, filter=f)
            st = case.idx.last_grouped_batch()
            print(f"{what} metric {metric}: {st}")
            assert st["routed"] == NQ and st["routed"] == st["settled"] + st["handed_back"], st
            check_rows(case, Q, k, metric, got, allowed=allowed, tag=what)
        assert not (set(got[1].ravel().tolist()) & set(case.ids[~allowed].tolist()))


def test_a_settled_batch_builds_no_position_list_for_an_exclusion_token(V, O):
    case, Q = shared_case(V, O, "eight_per_group", 12_345, 384)
    idx = case.idx
    idx.set_grouped_batch("on")
    with idx.make_filter([int(x) for x in case.ids[:50]], exclude=True) as f:
        got = idx.search_grouped_batch_arrays(Q, 1, COS, groups=case.table, filter=f)
        st = idx.last_grouped_batch()
        assert st["routed"] == NQ and st["settled"] == NQ, st  # the best row of random data clears the bound
        allowed = np.ones(case.ids.size, dtype=bool)
        allowed[:50] = False
        check_rows(case, Q, 1, COS, got, allowed=allowed)
        # the token's list does not exist yet: the next call that needs one builds it (what
        # test_a_certified_batch_builds_no_position_list of tests/test_gpu_masked_batch.py reads)
        idx.set_masked_batch("off")
        idx.search_batch(Q, 5, COS, filter=f)
        assert idx.last_masked_batch()["lists_built"] == 1
        idx.set_masked_batch("auto")


# ---- 4. the three modes; ineligible calls loop -------------------------------------------------------------------------------
def test_the_three_modes_return_identical_bits(V, O):
    case, Q = shared_case(V, O, "eight_per_group", 9_000, 128)
    idx = case.idx
    out = {}
    for mode in ("on", "off", "auto"):
        idx.set_grouped_batch(mode)
        out[mode] = idx.search_grouped_batch_arrays(Q, 10, COS, groups=case.table)
        st = idx.last_grouped_batch()
        if mode == "on":
            assert st["routed"] == NQ and st["settled"] > 0
        if mode == "off":
            assert st == {"routed": 0, "settled": 0, "handed_back": 0, "sequences": 0}
        assert st["routed"] in (0, NQ)
    for mode in ("off", "auto"):
        for a, b in zip(out["on"], out[mode]):
            assert a.tolist() == b.tolist() if a.dtype != np.float64 else bits(a) == bits(b), mode
    check_rows(case, Q, 10, COS, out["on"])
    idx.set_grouped_batch("on")
    with pytest.raises(KeyError):
        idx.set_grouped_batch("sometimes")


@pytest.mark.parametrize("why", ["Manhattan", "dim 1024", "k = 61", "one query", "8191 rows"])
def test_ineligible_calls_loop_and_match_the_single_call(V, O, why):
    n, dim, k, metric, nq = 9_000, 128, 10, COS, 4
    if why == "Manhattan":
        metric = MAN
    elif why == "dim 1024":
        dim = 1024
    elif why == "k = 61":
        k = 61
    elif why == "one query":
        nq = 1
    else:
        n = 8_191
    if dim == 128 and n == 9_000:
        case, Q = shared_case(V, O, "eight_per_group", n, dim)
    else:
        case, rng = make_case(V, O, "eight_per_group", dim, n, 77)
        Q = np.ascontiguousarray(queries_for(case, rng, "eight_per_group", count=4))
    Q = Q[:nq]
    case.idx.set_grouped_batch("on")
    got = case.idx.search_grouped_batch_arrays(Q, k, metric, groups=case.table)
    assert case.idx.last_grouped_batch() == {"routed": 0, "settled": 0, "handed_back": 0, "sequences": 0}
    equal_to_the_loop(case.idx, case.table, Q, k, metric, got, tag=why)
    check_rows(case, Q, k, metric, got, tag=why)


# ---- 5. fewer groups than k, small and empty S, NaN rows ---------------------------------------------------------------------
def test_fewer_groups_than_k_small_and_empty_s(V, O):
    rng = np.random.default_rng(51)
    n, dim = 9_000, 128
    ids = random_ids(rng, n)
    rows = unit_rows(rng, n, dim)
    Q = np.ascontiguousarray(rng.standard_normal((6, dim)))
    # a table of 7 groups over every row: the prefix never holds 10 groups, the single search answers with 7
    case7 = Case(V, O, dim, ids, rows, group_key(rng.integers(7, size=n) + 2))
    case7.idx.set_grouped_batch("on")
    got = case7.idx.search_grouped_batch_arrays(Q, 10, COS, groups=case7.table)
    st = case7.idx.last_grouped_batch()
    assert st["routed"] == 6 and st["handed_back"] == 6 and got[3].tolist() == [7] * 6, st
    check_rows(case7, Q, 10, COS, got)
    got = case7.idx.search_grouped_batch_arrays(Q, 3, COS, groups=case7.table)
    check_rows(case7, Q, 3, COS, got)
    # an S of 40 rows inside the 9 000-row index: the list holds all of S, settled with fewer than k groups
    has = np.zeros(n, dtype=bool)
    has[rng.choice(n, 40, replace=False)] = True
    gk = group_key(rng.integers(25, size=n) + 2)
    case40 = Case(V, O, dim, ids, rows, gk, has)
    case40.idx.set_grouped_batch("on")
    groups40 = len(set(gk[has].tolist()))
    for metric in MFMA_METRICS:
        got = case40.idx.search_grouped_batch_arrays(Q, 60, metric, groups=case40.table)
        st = case40.idx.last_grouped_batch()
        assert st == {"routed": 6, "settled": 6, "handed_back": 0, "sequences": 1}, st
        assert got[3].tolist() == [groups40] * 6
        check_rows(case40, Q, 60, metric, got)
    # the same S cut down to 3 rows by an include token, and to nothing by a token that shares no row with the table
    three = np.nonzero(has)[0][:3]
    allowed = np.zeros(n, dtype=bool)
    allowed[three] = True
    with case40.idx.make_filter(ids[three]) as f:
        got = case40.idx.search_grouped_batch_arrays(Q, 10, COS, groups=case40.table, filter=f)
        assert case40.idx.last_grouped_batch()["settled"] == 6
        check_rows(case40, Q, 10, COS, got, allowed=allowed)
    with case40.idx.make_filter(ids[~has][:100]) as f:
        got = case40.idx.search_grouped_batch_arrays(Q, 10, COS, groups=case40.table, filter=f)
        assert got[3].tolist() == [0] * 6
    with case40.idx.make_groups([2 ** 50 + 1, 2 ** 50 + 2], [1, 2]) as t:  # ids the index does not hold
        got = case40.idx.search_grouped_batch_arrays(Q, 10, COS, groups=t)
        assert got[3].tolist() == [0] * 6 and case40.idx.last_grouped_batch()["routed"] == 0
    # k = 0 and nq = 0
    got = case40.idx.search_grouped_batch_arrays(Q, 0, COS, groups=case40.table)
    assert got[0].shape == (6, 0) and got[3].tolist() == [0] * 6
    got = case40.idx.search_grouped_batch_arrays(np.zeros((0, dim)), 10, COS, groups=case40.table)
    assert got[0].shape == (0, 10) and got[3].shape == (0,)
    assert case40.idx.search_grouped_batch(np.zeros((0, dim)), 10, COS, groups=case40.table) == []
    res = case40.idx.search_grouped_batch(Q[:2], 3, COS, groups=case40.table)
    assert [len(r) for r in res] == [3, 3] and res[0][0][0] == int(case40.answer(Q[0], COS)[0][0])
    # argument errors: the single call's
    with pytest.raises(V.IndexOpError, match="VL_GROUPED_MAX_K"):
        case40.idx.search_grouped_batch_arrays(Q, 1025, COS, groups=case40.table)
    with pytest.raises(V.IndexOpError, match="unknown metric"):
        case40.idx.search_grouped_batch_arrays(Q, 5, 9, groups=case40.table)
    with pytest.raises(V.DimensionMismatch):
        case40.idx.search_grouped_batch_arrays(Q[:, :100], 5, COS, groups=case40.table)


def test_nan_rows_inside_and_outside_s(V, O):
    rng = np.random.default_rng(52)
    n, dim = 9_000, 128
    ids = random_ids(rng, n)
    rows = unit_rows(rng, n, dim)
    rows[10, 0] = np.nan
    rows[20, 3] = np.nan
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    idx.set_grouped_batch("on")
    Q = np.ascontiguousarray(rng.standard_normal((4, dim)))
    full = idx.make_groups(ids, group_key(np.arange(n) // 4 + 2))
    with pytest.raises(V.NaNScore):
        idx.search_grouped_batch_arrays(Q, 5, COS, groups=full)
    clean = np.ones(n, dtype=bool)
    clean[[10, 20]] = False
    with idx.make_groups(ids[clean], group_key(np.arange(n)[clean] // 4 + 2)) as t:  # the NaN rows have no group
        got = idx.search_grouped_batch_arrays(Q, 5, COS, groups=t)
        equal_to_the_loop(idx, t, Q, 5, COS, got)
        assert got[3].tolist() == [5] * 4 and not np.isnan(got[2]).any()
    with idx.make_filter(ids[clean]) as f:  # ... or are kept out by the filter
        got = idx.search_grouped_batch_arrays(Q, 5, COS, groups=full, filter=f)
        equal_to_the_loop(idx, full, Q, 5, COS, got, filt=f)
        assert not np.isnan(got[2]).any()


# ---- 6. table lifetime, threads, handles that refuse -------------------------------------------------------------------------
def test_the_table_follows_mutations_between_batches(V, O):
    rng = np.random.default_rng(61)
    n, dim, k = 9_000, 128, 10
    ids = random_ids(rng, n + 600)
    rows = unit_rows(rng, n + 600, dim)
    g = rng.integers(n // 8, size=n + 600) + 2
    has = rng.random(n + 600) < 0.6
    idx = V.FlatIndex(dim)
    idx.add_rows(ids[:n], rows[:n], validate=False)
    table = idx.make_groups(ids[has], group_key(g[has]))  # the pairs of rows that arrive later included
    idx.set_grouped_batch("on")
    Q = np.ascontiguousarray(rng.standard_normal((8, dim)))

    live = np.arange(n)

    def check(tag):
        ref = Case.__new__(Case)
        ref.V, ref.O, ref.dim = V, O, dim
        ref.ids, ref.rows, ref.gkeys, ref.has = ids[live], np.ascontiguousarray(rows[live]), group_key(g[live]), has[live]
        ref._answers, ref._refs = {}, {}
        got = idx.search_grouped_batch_arrays(Q, k, COS, groups=table)
        st = idx.last_grouped_batch()
        assert st["routed"] == 8 and st["settled"] > 0, (tag, st)
        check_rows(ref, Q, k, COS, got, tag=tag)
        assert table.rows() == int(has[live].sum())

    check("as built")
    idx.add_rows(ids[n:], rows[n:], validate=False)
    live = np.arange(n + 600)
    check("after add_rows")  # the cached bitmap is rebuilt: the new rows have groups
    gone = rng.choice(n + 600, 500, replace=False)
    assert idx.delete_many(ids[gone]) == 500
    live = np.setdiff1d(live, gone)
    check("after delete_many")
    moved = live[rng.choice(live.size, 300, replace=False)]
    rows[moved] = unit_rows(rng, 300, dim)
    idx.update_rows(ids[moved], rows[moved])
    check("after update_rows")


def test_four_threads_share_one_handle_with_two_tables(V, O):
    case, Q = shared_case(V, O, "eight_per_group", 9_000, 128)
    idx = case.idx
    idx.set_grouped_batch("on")
    other_keys = group_key(np.arange(case.ids.size) % 500 + 2)
    other = Case.__new__(Case)
    other.V, other.O, other.dim, other.ids, other.rows = V, O, case.dim, case.ids, case.rows
    other.gkeys, other.has, other._answers, other._refs = other_keys, np.ones(case.ids.size, dtype=bool), {}, {}
    other.table = idx.make_groups(case.ids, other_keys)
    expect = {0: [case.answer(q, COS) for q in Q], 1: [other.answer(q, COS) for q in Q]}
    errors = []

    def work(t):
        try:
            which = (case, other)[t % 2]
            for _ in range(4):
                keys, ids, scores, cnt = idx.search_grouped_batch_arrays(Q, 10, COS, groups=which.table)
                for i in range(len(Q)):
                    ek, ei, es = expect[t % 2][i]
                    assert cnt[i] == 10 and keys[i].tolist() == ek[:10] and ids[i].tolist() == ei[:10] and bits(scores[i]) == es[:10]
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_hnsw_and_multi_gpu_handles_refuse_and_a_short_stride_is_refused(V, O):
    rng = np.random.default_rng(2)
    Q = np.ascontiguousarray(rng.standard_normal((3, 8)))
    hn = V.HNSWIndex(8)
    hn.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        hn.search_grouped_batch_arrays(Q, 3, COS)
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        hn.search_grouped_batch(Q, 3, COS)
    mi = V.MultiFlatIndex(8, [0, 0])
    mi.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    n_out = np.zeros(3, dtype=np.uint64)
    buf, sc = np.zeros(24, dtype=np.uint64), np.zeros(24)
    for h in (hn._h, mi._h):
        rc = hn._L.vl_index_search_grouped_batch(h, 5, 0, Q.ctypes.data, 3, 8, 3, COS, 8, buf.ctypes.data, buf.ctypes.data,
                                                 sc.ctypes.data, n_out.ctypes.data)
        assert rc == V.VL_ERR_INVALID_ARG and b"single-GPU flat" in hn._L.vl_last_error()
        assert hn._L.vl_index_set_grouped_batch(h, 1) == V.VL_ERR_INVALID_ARG
        assert hn._L.vl_index_last_grouped_batch(h, None, None, None, None) == V.VL_ERR_INVALID_ARG
    # k > out_stride
    case, Qc = shared_case(V, O, "eight_per_group", 9_000, 128)
    keys = np.zeros(NQ * 10, dtype=np.uint64)
    ids = np.zeros(NQ * 10, dtype=np.uint64)
    scores = np.zeros(NQ * 10)
    cnt = np.zeros(NQ, dtype=np.uint64)
    rc = case.idx._L.vl_index_search_grouped_batch(case.idx._h, case.table.token, 0, Qc.ctypes.data, NQ, 128, 10, COS, 9,
                                                   keys.ctypes.data, ids.ctypes.data, scores.ctypes.data, cnt.ctypes.data)
    assert rc == V.VL_ERR_INVALID_ARG and b"out_stride" in case.idx._L.vl_last_error()
    rc = case.idx._L.vl_index_search_grouped_batch(case.idx._h, case.table.token, 0, Qc.ctypes.data, NQ, 128, 10, COS, 10,
                                                   keys.ctypes.data, ids.ctypes.data, scores.ctypes.data, cnt.ctypes.data)
    assert rc == 0 and cnt.tolist() == [10] * NQ
