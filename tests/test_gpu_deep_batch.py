"""The deep-k batch: search_batch with 60 < k <= VL_DEEP_MAX_K against the oracle's f64 scores -- the
top k by (score descending, position ascending), ids and score bits equal, the route's counters."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, EUC, DOT = 0, 1, 3
NQ = 24


@pytest.fixture(scope="module")
def V():
    import vectorlite_amd as V
    n_dev, _ = V.runtime_info()
    assert n_dev > 0, "GPU tests need a HIP device"
    return V


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64).tolist()


@functools.lru_cache(maxsize=2)
def stored(dim, n):
    rng = np.random.default_rng(34 * dim + n)
    return rng.standard_normal((n, dim)), np.arange(n, dtype=np.uint64) * np.uint64(10) + np.uint64(1)


def queries(dim):
    return np.random.default_rng(dim).standard_normal((NQ, dim))


def reference(rows, Q, k, metric):
    """Per query the (positions, scores) of its k best rows by (score desc, position asc)."""
    from oracle import oracle as O
    n = len(rows)
    ref = O.FlatOracle(rows.shape[1], np.arange(n, dtype=np.uint64), rows)
    out = []
    for q in Q:
        ri, rs = ref.search(q, n, metric)
        order = sorted(zip(ri.astype(np.int64).tolist(), rs.tolist()), key=lambda e: (-e[1], e[0]))[:k]
        out.append(([p for p, _ in order], [s for _, s in order]))
    return out


@functools.lru_cache(maxsize=3)
def case_reference(dim, n, metric):
    return reference(stored(dim, n)[0], queries(dim), 1024, metric)


_built = {}


def build(V, dim, n, rows=None):
    key = (dim, n, rows is None)
    if key not in _built:
        _built.clear()
        idx = V.FlatIndex(dim)
        idx.add_rows(stored(dim, n)[1], stored(dim, n)[0] if rows is None else rows, validate=False)
        _built[key] = idx
    return _built[key]


def check(idx, Q, k, metric, exp):
    ids, scores, cnt = idx.search_batch(Q, k, metric)
    assert cnt.tolist() == [k] * len(Q)
    for i, (pos, sc) in enumerate(exp):
        assert ids[i].tolist() == [10 * p + 1 for p in pos[:k]], (i, idx.last_deep_batch())
        assert bits(scores[i]) == bits(sc[:k]), (i, idx.last_deep_batch())
    return idx.last_deep_batch()


# strides 128, 384 and the phased 768; 8192 + 17 rows: a masked last block at the row floor, every row kept by the first
# stage at k = 1024; 40 000 rows: a spread sample with a striped first stage
@pytest.mark.parametrize("k", [61, 100, 1024])
@pytest.mark.parametrize("metric", [COS, EUC, DOT])
@pytest.mark.parametrize("n", [8192 + 17, 40000])
@pytest.mark.parametrize("dim", [100, 384, 768])
def test_deep_batch_equals_the_single_search(V, metric, dim, n, k):
    idx = build(V, dim, n)
    idx.set_deep_batch("on")
    routed, certified, back, seqs = check(idx, queries(dim), k, metric, case_reference(dim, n, metric))
    assert routed == NQ and certified + back == NQ and seqs == 1
    assert certified >= routed / 2  # the equality above must not rest on hand-backs alone


def test_several_stages_and_compactions(V, monkeypatch):
    monkeypatch.setenv("VL_DEEP_BATCH_FIRST_ROWS", "8192")  # stages end at 8192, 16 384, 32 768 and 40 000 rows
    idx = build(V, 384, 40000)
    for k in (61, 300):
        routed, certified, _, _ = check(idx, queries(384), k, COS, case_reference(384, 40000, COS))
        assert routed == NQ and certified >= routed / 2


def test_ties_zero_query_stored_row_and_switches(V, monkeypatch):
    dim, n, k = 100, 8192 + 17, 200
    rows = stored(dim, n)[0].copy()
    Q = queries(dim).copy()
    dup = np.random.default_rng(5).choice(n, size=300, replace=False)
    rows[dup] = Q[0] * 0.5        # 300 exact duplicates, the best rows of query 0: place k falls inside them
    Q[1] = 0.0                    # a zero query
    Q[2] = rows[77]               # a query equal to a stored row
    exp = reference(rows, Q, k, COS)
    assert set(exp[0][0]) < set(dup.tolist()) and exp[0][0] == sorted(exp[0][0])
    idx = build(V, dim, n, rows)
    routed, certified, back, _ = check(idx, Q, k, COS, exp)  # new handles: auto
    assert routed == NQ and back >= 1 and certified >= 1  # the zero query goes back
    assert check(idx, Q, 60, COS, exp)[0] == 0               # k = 60: the existing route, untouched
    idx.set_deep_batch("off")
    assert check(idx, Q, k, COS, exp) == (0, 0, 0, 0)
    idx.set_deep_batch("on")
    monkeypatch.setenv("VL_DEEP_BATCH_CAND_CAP", "256")      # lowered capacity: every query is handed back
    assert check(idx, Q, k, COS, exp)[:3] == (NQ, 0, NQ)
