"""Batched diversified search (vl_index_search_mmr_batch).  Row i of a batch is what the single MMR
search returns for query i: checked against the contract restated in Python (tests/test_gpu_mmr_search.py's Case: the
oracle's candidates, mmr_reference over the oracle's calculate) and, row for row, against the loop of single calls on the
same handle -- ids and score bits with ==, in selection order.  The parity cases also assert that the MFMA pass took the
batch, and the planted cases how many queries it settled: parity through hand-backs alone would prove nothing about it."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_mmr_search import Case, bits, random_ids  # noqa: E402

pytestmark = pytest.mark.gpu

COS, EUC, MAN, DOT = 0, 1, 2, 3
MFMA_METRICS = (COS, EUC, DOT)
SIZES = [(9_000, 128), (12_345, 384), (20_000, 768)]  # just above MFMA_MIN_ROWS = 8192, three kernel strides
K_FETCH = [(1, 1), (2, 2), (4, 20), (10, 60)]
LAMBDAS = (0.25, 0.5)
NQ = 12
ZERO = {"routed": 0, "settled": 0, "handed_back": 0, "sequences": 0}


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


def unit_rows(rng, n, dim):
    rows = rng.standard_normal((n, dim))
    return np.ascontiguousarray(rows / np.linalg.norm(rows, axis=1, keepdims=True))


_CASES = {}


def shared_case(V, O, n, dim):
    """one index, oracle and query set per size: the metrics share it and its candidate lists"""
    if (n, dim) not in _CASES:
        rng = np.random.default_rng(27 * dim + n)
        case = Case(V, O, dim, random_ids(rng, n), unit_rows(rng, n, dim))
        _CASES[(n, dim)] = (case, np.ascontiguousarray(rng.standard_normal((NQ, dim))))
    return _CASES[(n, dim)]


def check_rows(case, Q, k, fetch_k, lam, metric, got, positions=None, tag=None):
    ids, scores, cnt = got
    assert ids.shape == scores.shape == (len(Q), k) and cnt.shape == (len(Q),)
    reordered = 0
    for i, q in enumerate(Q):
        ei, es, sel = case.expect(q, k, fetch_k, lam, metric, positions)
        m = int(cnt[i])
        assert m == len(ei), (tag, metric, k, fetch_k, lam, i)
        assert ids[i, :m].tolist() == ei.tolist(), (tag, metric, k, fetch_k, lam, i)
        assert bits(scores[i, :m]) == bits(es), (tag, metric, k, fetch_k, lam, i)
        reordered += sel != list(range(len(sel)))
    return reordered


def equal_to_the_loop(idx, Q, k, fetch_k, lam, metric, got, filt=None, exclude=None, tag=None, rows=None):
    ids, scores, cnt = got
    for i in (range(len(Q)) if rows is None else rows):
        li, ls = idx.search_mmr_arrays(Q[i], k, fetch_k, lam, metric, filter=filt, exclude=exclude)
        m = int(cnt[i])
        assert m == li.size, (tag, i)
        assert ids[i, :m].tolist() == li.tolist(), (tag, i)
        assert bits(scores[i, :m]) == bits(ls), (tag, i)


def same_bits(a, b):
    return all((x.tolist() == y.tolist()) if x.dtype != np.float64 else (bits(x) == bits(y)) for x, y in zip(a, b))


# ---- 1. parity with the restated selection --------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", MFMA_METRICS)
@pytest.mark.parametrize("n,dim", SIZES)
def test_parity_with_the_restated_selection(V, O, n, dim, metric):
    case, Q = shared_case(V, O, n, dim)
    case.idx.set_mmr_batch("on")
    reordered = 0
    for k, fetch_k in K_FETCH:
        for lam in LAMBDAS:
            got = case.idx.search_mmr_batch_arrays(Q, k, fetch_k, lam, metric)
            st = case.idx.last_mmr_batch()
            print(f"{n} x {dim} metric {metric} (k, fetch_k) ({k}, {fetch_k}) lambda {lam}: {st}")
            assert st["routed"] == NQ and st["routed"] == st["settled"] + st["handed_back"], st
            assert st["sequences"] == 1
            reordered += check_rows(case, Q, k, fetch_k, lam, metric, got, tag=(n, dim))
            if metric == COS and fetch_k <= 20:
                # independent unit rows: the 20th score of thousands is far above the 64th key's bound; otherwise the parity
                # above proved nothing about the pass
                assert st["settled"] > 0, st
                assert V.last_path() == V.PATH_FAST
    assert reordered > 0  # redundancy actually reorders answers: the similarities matter


# ---- 2. row for row the loop of single calls: planted candidates ------------------------------------------------------------
def planted(rng, dim, n_background, nq, copies):
    """per query: 24 rows cos * q + sin * (unit noise orthogonal to q), cosines 0.95, 0.94, ... (copies = 0), or `copies`
    identical copies of the first such row, over gaussian background rows"""
    Q = unit_rows(rng, nq, dim)
    rows = [rng.standard_normal((n_background, dim))]
    for q in Q:
        block = []
        for c in (0.95 - 0.01 * np.arange(24) if copies == 0 else [0.95]):
            u = rng.standard_normal(dim)
            u -= (u @ q) * q
            u /= np.linalg.norm(u)
            block.append(c * q + np.sqrt(1.0 - c * c) * u)
        rows.append(np.array(block) if copies == 0 else np.repeat(np.array(block), copies, axis=0))
    rows = np.ascontiguousarray(np.vstack(rows))
    return rng.permutation(rows), np.ascontiguousarray(Q)


def test_planted_candidates_are_settled_by_the_pass(V, O):
    rng = np.random.default_rng(271)
    rows, Q = planted(rng, 128, 9_000, 6, 0)
    idx = V.FlatIndex(128)
    idx.add_rows(random_ids(rng, len(rows)), rows, validate=False)
    idx.set_mmr_batch("on")
    for lam in (0.0, 0.5, 1.0):
        got = idx.search_mmr_batch_arrays(Q, 4, 20, lam, COS)
        st = idx.last_mmr_batch()
        print(f"planted lambda {lam}: {st}")
        # a condition, not a measurement: the 20th score (0.76) is about 0.3 above the 64th key, far outside any bf16 bound
        assert st["routed"] == len(Q) and st["settled"] == len(Q) and st["handed_back"] == 0, st
        assert V.last_path() == V.PATH_FAST
        equal_to_the_loop(idx, Q, 4, 20, lam, COS, got, tag=("planted", lam))
        assert got[2].tolist() == [4] * len(Q)
    got = idx.search_mmr_batch_arrays(Q, 20, 20, 0.5, COS)
    assert idx.last_mmr_batch()["settled"] == len(Q)
    equal_to_the_loop(idx, Q, 20, 20, 0.5, COS, got, tag="planted (20, 20)")


def test_tied_candidates_are_handed_back(V, O):
    rng = np.random.default_rng(272)
    rows, Q = planted(rng, 128, 9_000, 6, 100)
    idx = V.FlatIndex(128)
    idx.add_rows(random_ids(rng, len(rows)), rows, validate=False)
    idx.set_mmr_batch("on")
    got = idx.search_mmr_batch_arrays(Q, 4, 20, 0.5, COS)
    st = idx.last_mmr_batch()
    print(f"tied: {st}")
    # all 64 listed scores equal the bound's key: nothing is strictly above it
    assert st["routed"] == len(Q) and st["handed_back"] == len(Q) and st["settled"] == 0, st
    equal_to_the_loop(idx, Q, 4, 20, 0.5, COS, got, tag="tied")


# ---- 3. filters of both kinds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["include 1 %", "include 30 %", "include 100 %", "exclude 0", "exclude 50", "exclude 5000"])
def test_filters_of_both_kinds(V, O, what):
    n, dim = 12_345, 384
    case, Q = shared_case(V, O, n, dim)
    case.idx.set_mmr_batch("on")
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
    positions = np.nonzero(allowed)[0].astype(np.uint64)
    with f:
        for metric in MFMA_METRICS:
            got = case.idx.search_mmr_batch_arrays(Q, 4, 20, 0.5, metric, filter=f)
            st = case.idx.last_mmr_batch()
            print(f"{what} metric {metric}: {st}")
            assert st["routed"] == NQ and st["routed"] == st["settled"] + st["handed_back"], st
            check_rows(case, Q, 4, 20, 0.5, metric, got, positions=positions, tag=what)
            if metric == COS:
                assert st["settled"] > 0, st
        assert not (set(got[0].ravel().tolist()) & set(case.ids[~allowed].tolist()))
        equal_to_the_loop(case.idx, Q, 4, 20, 0.5, COS, case.idx.search_mmr_batch_arrays(Q, 4, 20, 0.5, COS, filter=f), filt=f, tag=what)


def test_a_settled_batch_builds_no_position_list_for_an_exclusion_token(V, O):
    case, Q = shared_case(V, O, 12_345, 384)
    idx = case.idx
    idx.set_mmr_batch("on")
    with idx.make_filter([int(x) for x in case.ids[:50]], exclude=True) as f:
        got = idx.search_mmr_batch_arrays(Q, 1, 1, 0.5, COS, filter=f)
        st = idx.last_mmr_batch()
        assert st["routed"] == NQ and st["settled"] == NQ, st  # the best row of random data clears the bound
        check_rows(case, Q, 1, 1, 0.5, COS, got, positions=np.arange(50, case.ids.size, dtype=np.uint64))
        # the token's list does not exist yet: the next call that needs one builds it (what
        # test_a_certified_batch_builds_no_position_list of tests/test_gpu_masked_batch.py reads)
        idx.set_masked_batch("off")
        idx.search_batch(Q, 5, COS, filter=f)
        assert idx.last_masked_batch()["lists_built"] == 1
        idx.set_masked_batch("auto")


# ---- 4. the three modes; ineligible calls loop -------------------------------------------------------------------------------
def test_the_three_modes_return_identical_bits(V, O):
    case, Q = shared_case(V, O, 9_000, 128)
    idx = case.idx
    out = {}
    for mode in ("on", "off", "auto"):
        idx.set_mmr_batch(mode)
        out[mode] = idx.search_mmr_batch_arrays(Q, 4, 20, 0.5, COS)
        st = idx.last_mmr_batch()
        if mode == "on":
            assert st["routed"] == NQ and st["settled"] > 0
        if mode == "off":
            assert st == ZERO
        assert st["routed"] in (0, NQ)
    assert same_bits(out["on"], out["off"]) and same_bits(out["on"], out["auto"])
    check_rows(case, Q, 4, 20, 0.5, COS, out["on"])
    idx.set_mmr_batch("on")
    with pytest.raises(KeyError):
        idx.set_mmr_batch("sometimes")
    # an unknown mode is refused by the library and leaves the mode as it was; nq = 0 writes nothing
    assert idx._L.vl_index_set_mmr_batch(idx._h, 3) == V.VL_ERR_INVALID_ARG and idx._L.vl_index_set_mmr_batch(idx._h, -1) == V.VL_ERR_INVALID_ARG
    assert same_bits(idx.search_mmr_batch_arrays(Q, 4, 20, 0.5, COS), out["on"]) and idx.last_mmr_batch()["routed"] == NQ
    cnt = np.full(2, 77, dtype=np.uint64)
    assert idx._L.vl_index_search_mmr_batch(idx._h, 0, Q.ctypes.data, 0, 128, 4, 20, 0.5, COS, 4, None, None, cnt.ctypes.data) == 0
    assert cnt.tolist() == [77, 77] and idx.last_mmr_batch() == ZERO


@pytest.mark.parametrize("why", ["Manhattan", "dim 1024", "fetch_k = 61", "one query", "8191 rows"])
def test_ineligible_calls_loop_and_match_the_single_call(V, O, why):
    n, dim, k, fetch_k, metric, nq = 9_000, 128, 4, 20, COS, 4
    if why == "Manhattan":
        metric = MAN
    elif why == "dim 1024":
        dim = 1024
    elif why == "fetch_k = 61":
        k, fetch_k = 10, 61
    elif why == "one query":
        nq = 1
    else:
        n = 8_191
    if dim == 128 and n == 9_000:
        case, Q = shared_case(V, O, n, dim)
    else:
        rng = np.random.default_rng(77)
        case = Case(V, O, dim, random_ids(rng, n), unit_rows(rng, n, dim))
        Q = np.ascontiguousarray(rng.standard_normal((4, dim)))
    Q = Q[:nq]
    case.idx.set_mmr_batch("on")
    got = case.idx.search_mmr_batch_arrays(Q, k, fetch_k, 0.5, metric)
    assert case.idx.last_mmr_batch() == ZERO
    equal_to_the_loop(case.idx, Q, k, fetch_k, 0.5, metric, got, tag=why)
    check_rows(case, Q, k, fetch_k, 0.5, metric, got, tag=why)


# ---- 5. small and empty subsets, k = 0, a short stride, NaN rows ---------------------------------------------------------------
def test_small_and_empty_subsets_and_k_zero(V, O):
    case, Q = shared_case(V, O, 9_000, 128)
    idx = case.idx
    idx.set_mmr_batch("on")
    rng = np.random.default_rng(51)
    for m in (5, 40, 64, 65):
        positions = np.sort(rng.choice(9_000, m, replace=False)).astype(np.uint64)
        with idx.make_filter(case.ids[positions.astype(np.int64)]) as f:
            for k, fetch_k in ((4, 20), (10, 60)):
                for metric in MFMA_METRICS:
                    got = idx.search_mmr_batch_arrays(Q, k, fetch_k, 0.5, metric, filter=f)
                    st = idx.last_mmr_batch()
                    print(f"m {m} ({k}, {fetch_k}) metric {metric}: {st}")
                    assert st["routed"] == NQ and st["routed"] == st["settled"] + st["handed_back"], st
                    if m <= 64:
                        assert st["settled"] == NQ, st  # the list holds all of S: every candidate is certified
                    assert got[2].tolist() == [min(k, m)] * NQ
                    check_rows(case, Q, k, fetch_k, 0.5, metric, got, positions=positions, tag=("small", m))
    # an empty S: a token none of whose ids the index holds, and an exclusion token that keeps nothing
    with idx.make_filter([2 ** 50 + 1, 2 ** 50 + 2]) as f:
        got = idx.search_mmr_batch_arrays(Q, 4, 20, 0.5, COS, filter=f)
        assert got[2].tolist() == [0] * NQ and idx.last_mmr_batch() == ZERO
    with idx.make_filter(case.ids, exclude=True) as f:
        got = idx.search_mmr_batch_arrays(Q, 4, 20, 0.5, COS, filter=f)
        assert got[2].tolist() == [0] * NQ and idx.last_mmr_batch() == ZERO
    # k = 0 and nq = 0
    got = idx.search_mmr_batch_arrays(Q, 0, 20, 0.5, COS)
    assert got[0].shape == (NQ, 0) and got[2].tolist() == [0] * NQ
    got = idx.search_mmr_batch_arrays(np.zeros((0, 128)), 4, 20, 0.5, COS)
    assert got[0].shape == (0, 4) and got[2].shape == (0,)
    assert idx.search_mmr_batch(np.zeros((0, 128)), 4, 20, 0.5, COS) == []
    res = idx.search_mmr_batch(Q[:2], 3, 20, 0.5, COS)
    assert [len(r) for r in res] == [3, 3] and res[0][0].id == int(case.expect(Q[0], 3, 20, 0.5, COS)[0][0])
    # argument errors: the single call's
    with pytest.raises(V.IndexOpError, match="lambda"):
        idx.search_mmr_batch_arrays(Q, 4, 20, 1.5, COS)
    with pytest.raises(V.IndexOpError, match="fetch_k must be at least k"):
        idx.search_mmr_batch_arrays(Q, 21, 20, 0.5, COS)
    with pytest.raises(V.IndexOpError, match="unknown metric"):
        idx.search_mmr_batch_arrays(Q, 4, 20, 0.5, 9)
    # an unknown filter token: the single call's status and text, before the metric is looked at
    cnt, one = np.zeros(NQ, dtype=np.uint64), C.c_uint64(0)
    buf, sc = np.zeros(NQ * 4, dtype=np.uint64), np.zeros(NQ * 4)
    rc = idx._L.vl_index_search_mmr_batch(idx._h, 2 ** 60, Q.ctypes.data, NQ, 128, 4, 20, 0.5, 9, 4, buf.ctypes.data, sc.ctypes.data,
                                          cnt.ctypes.data)
    msg = idx._L.vl_last_error()
    rc1 = idx._L.vl_index_search_mmr(idx._h, 2 ** 60, Q.ctypes.data, 128, 4, 20, 0.5, 9, 4, buf.ctypes.data, sc.ctypes.data, C.byref(one))
    assert rc == rc1 == V.VL_ERR_INVALID_ARG and msg == idx._L.vl_last_error() and b"metric" not in msg
    with pytest.raises(V.DimensionMismatch):
        idx.search_mmr_batch_arrays(Q[:, :100], 4, 20, 0.5, COS)


def test_a_short_stride_gives_the_prefix_and_guard_words_stay(V, O):
    case, Q = shared_case(V, O, 9_000, 128)
    idx, L = case.idx, case.idx._L
    idx.set_mmr_batch("on")
    full = idx.search_mmr_batch_arrays(Q, 4, 20, 0.5, COS)
    assert idx.last_mmr_batch()["settled"] > 0
    GUARD = 0xA5A5A5A5A5A5A5A5

    def raw(k, stride, token=0):
        ids = np.full(NQ * stride + 8, GUARD, dtype=np.uint64)
        scores = np.full(NQ * stride + 8, GUARD, dtype=np.uint64)
        cnt = np.zeros(NQ, dtype=np.uint64)
        rc = L.vl_index_search_mmr_batch(idx._h, token, Q.ctypes.data, NQ, 128, k, 20, 0.5, COS, stride, ids.ctypes.data,
                                         scores.ctypes.data, cnt.ctypes.data)
        assert rc == 0
        return ids, scores, cnt

    # out_stride 3 < k 4: the first three of the four, as the single call with capacity 3 answers
    ids, scores, cnt = raw(4, 3)
    assert cnt.tolist() == [3] * NQ
    assert ids[:NQ * 3].reshape(NQ, 3).tolist() == full[0][:, :3].tolist()
    assert scores[:NQ * 3].reshape(NQ, 3).tolist() == full[1][:, :3].view(np.uint64).tolist()
    assert ids[NQ * 3:].tolist() == [GUARD] * 8 and scores[NQ * 3:].tolist() == [GUARD] * 8
    # out_stride 6 > k 4: entries 4 and 5 of every row are not written
    ids, scores, cnt = raw(4, 6)
    assert cnt.tolist() == [4] * NQ
    assert ids[:NQ * 6].reshape(NQ, 6)[:, :4].tolist() == full[0].tolist()
    assert ids[:NQ * 6].reshape(NQ, 6)[:, 4:].tolist() == [[GUARD, GUARD]] * NQ
    assert scores[:NQ * 6].reshape(NQ, 6)[:, 4:].tolist() == [[GUARD, GUARD]] * NQ
    assert ids[NQ * 6:].tolist() == [GUARD] * 8
    # ... and a row whose S has two rows holds two entries
    with idx.make_filter(case.ids[[7, 4000]]) as f:
        ids, scores, cnt = raw(4, 6, f.token)
        assert cnt.tolist() == [2] * NQ
        assert ids[:NQ * 6].reshape(NQ, 6)[:, 2:].tolist() == [[GUARD] * 4] * NQ
        assert set(ids[:NQ * 6].reshape(NQ, 6)[:, :2].ravel().tolist()) == {int(case.ids[7]), int(case.ids[4000])}
    # out_stride 0: zeros
    cnt = np.full(NQ, 9, dtype=np.uint64)
    assert L.vl_index_search_mmr_batch(idx._h, 0, Q.ctypes.data, NQ, 128, 4, 20, 0.5, COS, 0, None, None, cnt.ctypes.data) == 0
    assert cnt.tolist() == [0] * NQ


def test_nan_rows_inside_and_outside_s(V, O):
    rng = np.random.default_rng(52)
    n, dim = 9_000, 128
    ids = random_ids(rng, n)
    rows = unit_rows(rng, n, dim)
    rows[10, 0] = np.nan
    rows[20, 3] = np.nan
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    idx.set_mmr_batch("on")
    Q = np.ascontiguousarray(rng.standard_normal((4, dim)))
    with pytest.raises(V.NaNScore):
        idx.search_mmr_batch_arrays(Q, 4, 20, 0.5, COS)
    # the status of the LOWEST failing query: query 0 fails on a NaN score before query 1's ... every query fails alike
    # here, so the raw status is the single call's
    one = C.c_uint64(0)
    buf, sc = np.zeros(8, dtype=np.uint64), np.zeros(8)
    rc1 = idx._L.vl_index_search_mmr(idx._h, 0, Q.ctypes.data, dim, 4, 20, 0.5, COS, 4, buf.ctypes.data, sc.ctypes.data, C.byref(one))
    cnt = np.zeros(4, dtype=np.uint64)
    out_i, out_s = np.zeros(16, dtype=np.uint64), np.zeros(16)
    rcb = idx._L.vl_index_search_mmr_batch(idx._h, 0, Q.ctypes.data, 4, dim, 4, 20, 0.5, COS, 4, out_i.ctypes.data, out_s.ctypes.data,
                                           cnt.ctypes.data)
    assert rcb == rc1 != 0
    clean = np.ones(n, dtype=bool)
    clean[[10, 20]] = False
    with idx.make_filter(ids[clean]) as f:  # the NaN rows are kept out by an include token ...
        got = idx.search_mmr_batch_arrays(Q, 4, 20, 0.5, COS, filter=f)
        equal_to_the_loop(idx, Q, 4, 20, 0.5, COS, got, filt=f)
        assert got[2].tolist() == [4] * 4 and not np.isnan(got[1]).any()
    with idx.make_filter(ids[~clean], exclude=True) as f:  # ... or by an exclusion token
        got = idx.search_mmr_batch_arrays(Q, 4, 20, 0.5, COS, filter=f)
        equal_to_the_loop(idx, Q, 4, 20, 0.5, COS, got, filt=f)
        assert not np.isnan(got[1]).any()


def test_a_failing_query_behind_settled_ones_decides_the_status(V, O):
    """Clean rows, so the batch takes the pass: queries 0 .. 2 are settled there, query 3 (a NaN component: outside the
    fast-path domain) is handed back and its single call fails, query 4 is never reached.  The call returns query 3's own
    status; with a valid query in its place the same batch succeeds."""
    case, Q = shared_case(V, O, 9_000, 128)
    idx, L = case.idx, case.idx._L
    idx.set_mmr_batch("on")
    bad = np.ascontiguousarray(Q[:5].copy())
    bad[3, 7] = np.nan
    bad[4, 0] = np.nan
    one = C.c_uint64(0)
    buf, sc = np.zeros(8, dtype=np.uint64), np.zeros(8)
    rc_single = L.vl_index_search_mmr(idx._h, 0, bad[3].ctypes.data, 128, 4, 20, 0.5, COS, 4, buf.ctypes.data, sc.ctypes.data, C.byref(one))
    assert rc_single != 0
    cnt = np.zeros(5, dtype=np.uint64)
    out_i, out_s = np.zeros(20, dtype=np.uint64), np.zeros(20)
    rc = L.vl_index_search_mmr_batch(idx._h, 0, bad.ctypes.data, 5, 128, 4, 20, 0.5, COS, 4, out_i.ctypes.data, out_s.ctypes.data,
                                     cnt.ctypes.data)
    assert rc == rc_single
    # the queries in front of the failing one were answered by the pass before the hand-back ran
    good = idx.search_mmr_batch_arrays(Q[:5], 4, 20, 0.5, COS)
    assert idx.last_mmr_batch()["settled"] == 5
    assert cnt[:3].tolist() == [4, 4, 4] and out_i[:12].reshape(3, 4).tolist() == good[0][:3].tolist()
    with pytest.raises(V.NaNScore):
        idx.search_mmr_batch_arrays(bad, 4, 20, 0.5, COS)


# ---- 6. two launch sequences -------------------------------------------------------------------------------------------------
def test_two_launch_sequences_use_both_result_block_slots(V, O):
    case, _ = shared_case(V, O, 9_000, 128)
    idx = case.idx
    idx.set_mmr_batch("on")
    rng = np.random.default_rng(61)
    big = np.ascontiguousarray(rng.standard_normal((2048 + 3, 128)))
    # queries per launch sequence at this dimension (mfma_sequence_queries): 2048 queries are cut into whole sequences
    idx.search_mmr_batch_arrays(big[:2048], 4, 20, 0.5, COS)
    seq = 2048 // idx.last_mmr_batch()["sequences"]
    assert seq * idx.last_mmr_batch()["sequences"] == 2048
    Q = big[:seq + 3]
    got = idx.search_mmr_batch_arrays(Q, 4, 20, 0.5, COS)
    st = idx.last_mmr_batch()
    print(f"{seq} queries per sequence: {st}")
    # sequence 0 writes result-block slot 0, sequence 1 (the last three queries) slot 1
    assert st["sequences"] == 2 and st["routed"] == seq + 3 and st["routed"] == st["settled"] + st["handed_back"], st
    assert st["settled"] > seq  # queries of both slots were settled
    rows = list(range(4)) + list(range(seq - 3, seq + 3))
    equal_to_the_loop(idx, Q, 4, 20, 0.5, COS, got, rows=rows, tag="two sequences")
    # lambda = 1 is the plain top k: every row against the top-k batch
    got = idx.search_mmr_batch_arrays(Q, 4, 20, 1.0, COS)
    ti, ts = idx.search_batch(Q, 4, COS)[:2]
    assert got[0].tolist() == np.asarray(ti).reshape(len(Q), 4).tolist()
    assert bits(got[1]) == bits(np.asarray(ts).reshape(len(Q), 4))


# ---- 7. mutations between batches, threads, handles that refuse ---------------------------------------------------------------
def test_the_batch_follows_mutations_between_calls(V, O):
    rng = np.random.default_rng(71)
    n, dim = 9_000, 128
    ids = random_ids(rng, n + 600)
    rows = unit_rows(rng, n + 600, dim)
    idx = V.FlatIndex(dim)
    idx.add_rows(ids[:n], rows[:n], validate=False)
    idx.set_mmr_batch("on")
    Q = np.ascontiguousarray(rng.standard_normal((8, dim)))
    keep_out = ids[rng.choice(n + 600, 300, replace=False)]
    f = idx.make_filter(keep_out, exclude=True)

    def check(tag):
        for filt in (None, f):
            got = idx.search_mmr_batch_arrays(Q, 4, 20, 0.5, COS, filter=filt)
            st = idx.last_mmr_batch()
            assert st["routed"] == 8 and st["settled"] > 0, (tag, st)
            equal_to_the_loop(idx, Q, 4, 20, 0.5, COS, got, filt=filt, tag=tag)
            if filt is not None:
                assert not (set(got[0].ravel().tolist()) & set(keep_out.tolist()))

    check("as built")
    idx.add_rows(ids[n:], rows[n:], validate=False)
    check("after add_rows")
    gone = rng.choice(n + 600, 500, replace=False)
    assert idx.delete_many(ids[gone]) == 500
    check("after delete_many")
    live = np.setdiff1d(np.arange(n + 600), gone)
    moved = live[rng.choice(live.size, 300, replace=False)]
    rows[moved] = unit_rows(rng, 300, dim)
    idx.update_rows(ids[moved], rows[moved])
    check("after update_rows")
    f.close()


def test_four_threads_share_one_handle(V, O):
    case, Q = shared_case(V, O, 9_000, 128)
    idx = case.idx
    idx.set_mmr_batch("on")
    expect = {lam: idx.search_mmr_batch_arrays(Q, 4, 20, lam, COS) for lam in (0.25, 0.5)}
    for lam in expect:
        check_rows(case, Q, 4, 20, lam, COS, expect[lam])
    errors = []

    def work(t):
        try:
            lam = (0.25, 0.5)[t % 2]
            for _ in range(4):
                assert same_bits(idx.search_mmr_batch_arrays(Q, 4, 20, lam, COS), expect[lam])
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_hnsw_and_multi_gpu_handles_refuse(V, O):
    rng = np.random.default_rng(2)
    Q = np.ascontiguousarray(rng.standard_normal((3, 8)))
    hn = V.HNSWIndex(8)
    hn.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        hn.search_mmr_batch_arrays(Q, 3, 5, 0.5, COS)
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        hn.search_mmr_batch(Q, 3, 5, 0.5, COS)
    mi = V.MultiFlatIndex(8, [0, 0])
    mi.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        mi.search_mmr_batch_arrays(Q, 3, 5, 0.5, COS)
    n_out = np.zeros(3, dtype=np.uint64)
    buf, sc = np.zeros(24, dtype=np.uint64), np.zeros(24)
    for h in (hn._h, mi._h):
        rc = hn._L.vl_index_search_mmr_batch(h, 0, Q.ctypes.data, 3, 8, 3, 5, 0.5, COS, 8, buf.ctypes.data, sc.ctypes.data,
                                             n_out.ctypes.data)
        assert rc == V.VL_ERR_INVALID_ARG and b"single-GPU flat" in hn._L.vl_last_error()
        assert hn._L.vl_index_set_mmr_batch(h, 1) == V.VL_ERR_INVALID_ARG
        assert hn._L.vl_index_last_mmr_batch(h, None, None, None, None) == V.VL_ERR_INVALID_ARG
