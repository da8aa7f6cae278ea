"""The k-nearest-neighbour graph (vl_index_knn_graph) against brute force over the oracle's f64 score of
every pair (row p as the query): per row every other position ranked by (score desc with -0.0 == +0.0, position asc), cut at
kk.  Neighbour ids and score bits are compared; no tolerances.  The MFMA cases demand the MFMA route."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, EUC, MAN, DOT = 0, 1, 2, 3


@pytest.fixture(scope="module")
def V():
    import vectorlite_amd as V
    n_dev, _ = V.runtime_info()
    assert n_dev > 0, "GPU tests need a HIP device"
    return V


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64).tolist()


@functools.lru_cache(maxsize=None)
def planted(n, dim, clump=False):
    """Gaussian directions 0.25 .. 4 long.  Rows 0, 48 and n - 2 identical (the first position, a chunk edge at every stride,
    the partial last block), row 3 zero, near-duplicates across (63, 64) -- a 32-row block edge and the 64-row chunk edge --
    and (95, 96), the 48-row chunk's.  clump: rows 100 .. 160 are near-copies of one direction, which no bound tells apart."""
    rng = np.random.default_rng(1000 * n + dim)
    rows = rng.standard_normal((n, dim)) * rng.uniform(0.25, 4.0, (n, 1))
    if clump:
        rows[100:161] = rows[100] + 1e-3 * rng.standard_normal((61, dim))
    for a, b in ((63, 64), (95, 96)):
        if b < n:
            rows[b] = 1.7 * rows[a] + 0.05 * rng.standard_normal(dim)
    if n > 4:
        rows[3] = 0.0
        rows[min(48, n // 2)] = rows[0]
        rows[n - 2] = rows[0]
    return np.ascontiguousarray(rows)


def pair_scores(rows, metric):
    from oracle import oracle as O
    n, dim = rows.shape
    ref = O.FlatOracle(dim, np.arange(n, dtype=np.uint64), rows)
    S = np.empty((n, n))
    for i in range(n):
        ri, rs = ref.search(rows[i], n, metric)
        S[i, ri.astype(np.int64)] = rs
    return S


@functools.lru_cache(maxsize=None)
def scores_of(n, dim, metric, clump=False):
    return pair_scores(planted(n, dim, clump), metric)


def expected(S, k):
    n = len(S)
    kk = min(k, n - 1)
    pos = np.empty((n, kk), dtype=np.int64)
    for p in range(n):
        order = np.lexsort((np.arange(n), -(S[p] + 0.0)))
        pos[p] = order[order != p][:kk]
    return pos, np.take_along_axis(S, pos, axis=1)


def ids_for(n):  # ids carry no order and repeat: duplicate ids are distinct rows
    return np.random.default_rng(n).permutation(n).astype(np.uint64) * np.uint64(7) % np.uint64(max(n - 1, 1))


_built = {}


def build(V, n, dim, clump=False):
    key = (n, dim, clump)
    if key not in _built:
        _built.clear()
        idx = V.FlatIndex(dim)
        idx.add_rows(ids_for(n), planted(*key), validate=False)
        _built[key] = idx
    return _built[key]


def check(V, idx, ids, S, k, metric, route="mfma"):
    pos, sc = expected(S, k)
    got_ids, nbr, got_sc = idx.knn_graph(k, metric)
    lk = idx.last_knn()
    assert lk["route"] == route and V.last_path() == (V.PATH_FAST if route == "mfma" else V.PATH_EXACT_SORT), lk
    assert got_ids.tolist() == ids.tolist() and nbr.shape == pos.shape
    assert nbr.tolist() == ids[pos].tolist(), (k, metric, lk)
    assert bits(got_sc.ravel()) == bits(sc.ravel()), (k, metric, lk)
    return lk


@pytest.mark.parametrize("metric", [COS, EUC, DOT])
@pytest.mark.parametrize("n,dim", [(2, 384), (33, 384), (129, 384), (274, 384), (274, 100), (274, 768)])
def test_mfma_route_matches_brute_force(V, n, dim, metric):
    idx, ids, S = build(V, n, dim), ids_for(n), scores_of(n, dim, metric)
    for k in (1, 10, 32):
        if k <= n - 1:
            lk = check(V, idx, ids, S, k, metric)
            assert lk["seeds"] == n * k and lk["kept"] >= n * k and lk["split"] == 0 and lk["exact_rows"] == 0, lk
        else:  # every row keeps every other row: the exact route answers
            check(V, idx, ids, S, k, metric, route="exact")


@pytest.mark.parametrize("metric,route", [(MAN, "auto"), (COS, "exact"), (EUC, "exact")])
def test_exact_route(V, metric, route):
    idx = build(V, 129, 384)
    idx.set_knn_route(route)
    try:
        lk = check(V, idx, ids_for(129), scores_of(129, 384, metric), 10, metric, route="exact")
    finally:
        idx.set_knn_route("auto")
    assert lk["exact_rows"] == 129


def test_a_small_candidate_buffer_splits_ranges_and_hands_a_block_over(V, monkeypatch):
    """k = 1 and a buffer of 300 pairs: first ranges of two blocks.  The 61 clump rows keep 60 partners each, so their ranges
    split and their blocks go to the exact route; the gaussian blocks keep a few pairs per row and stay on the pass."""
    idx = build(V, 274, 384, True)
    monkeypatch.setenv("VL_KNN_CAND_CAP", "300")
    lk = check(V, idx, ids_for(274), scores_of(274, 384, COS, True), 1, COS)
    assert lk["split"] > 0 and 61 <= lk["exact_rows"] < 274 and lk["seeds"] > 0, lk
    monkeypatch.setenv("VL_KNN_CAND_CAP", "1")  # clamped to 32 k: every block with one pair beyond its seeds is handed over
    check(V, idx, ids_for(274), scores_of(274, 384, COS, True), 10, COS)


def test_nan_row_then_delete_and_add(V):
    rows = planted(129, 100)
    idx = V.FlatIndex(100)
    idx.add_rows(np.arange(129, dtype=np.uint64), rows, validate=False)
    idx.add_rows(np.array([999], dtype=np.uint64), np.full((1, 100), np.nan), validate=False)
    with pytest.raises(V.NaNScore):
        idx.knn_graph(5, COS)
    idx.delete(999)
    idx.delete_many(np.array([0, 64, 100], dtype=np.uint64))
    idx.add_rows(np.arange(500, 507, dtype=np.uint64), planted(33, 100)[5:12], validate=False)
    ids, vals = idx.export()
    assert len(ids) == 133
    check(V, idx, ids, pair_scores(vals, EUC), 10, EUC)


def test_argument_errors_small_indexes_and_refusals(V):
    idx = V.FlatIndex(384)
    for n in (0, 1):
        ids, nbr, sc = idx.knn_graph(3)
        assert len(ids) == n and nbr.shape == (n, 0) and sc.shape == (n, 0)
        idx.add_rows(np.array([5], dtype=np.uint64), np.ones((1, 384)), validate=False)
    for k, metric in ((0, COS), (33, COS), (0, 9), (3, 9)):
        with pytest.raises(V.IndexOpError):
            idx.knn_graph(k, metric)
    with pytest.raises(ValueError):
        idx.set_knn_route("fast")
    for other in (V.HNSWIndex(384), V.MultiFlatIndex(8, [0, 0])):
        for call in (lambda: other.knn_graph(3), lambda: other.set_knn_route("exact"), other.last_knn):
            with pytest.raises(V.IndexOpError, match="single-GPU flat"):
                call()
