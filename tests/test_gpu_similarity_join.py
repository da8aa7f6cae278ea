"""The similarity self-join (vl_index_similarity_join) against brute force: the oracle's f64 score of
every pair (row i as the query, as the contract defines it), cut at the threshold and ordered (score desc, i, j) in Python.
The MFMA cases demand the MFMA route with no panel handed back: a case the fallback answered says nothing about the kernel."""
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


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O
    return O


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64).tolist()


def planted_rows(n, dim, seed):
    """Unit-variance gaussian rows with near-duplicates planted (a, b, cosine): inside one 16-row group, across a 32-row block
    edge, across the 128- and 96-row panel edges, first and last row, the partial last block; rows 5, 6, 7 identical."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, dim))
    used, pairs = set(), []
    plan = [(0, n - 1, 0.85), (3, 9, 0.99), (31, 32, 0.78), (127, 128, 0.85), (95, 96, 0.85), (5, 6, 1.0), (5, 7, 1.0),
            (n - 3, n - 2, 0.99), (200, 40, 0.78)]
    for a, b, c in plan:
        if min(a, b) < 0 or max(a, b) >= n or a == b or b in used or (a in used and c != 1.0):
            continue
        ua = rows[a] / np.linalg.norm(rows[a])
        w = rng.standard_normal(dim)
        w -= (w @ ua) * ua
        w /= np.linalg.norm(w)
        rows[b] = rows[a] if c == 1.0 else (c * ua + np.sqrt(1.0 - c * c) * w) * rng.uniform(0.5, 3.0)
        used.update((a, b))
        pairs.append((min(a, b), max(a, b)))
    return rows, pairs


def pair_scores(O, rows, metric):
    """S[i, j] = the reference score search_range(query = row i) reports for position j."""
    n, dim = rows.shape
    ref = O.FlatOracle(dim, np.arange(n, dtype=np.uint64), rows)
    S = np.empty((n, n))
    for i in range(n):
        ri, rs = ref.search(rows[i], n, metric)
        S[i, ri.astype(np.int64)] = rs
    return S


def expected(S, min_score):
    i, j = np.nonzero(np.triu(S >= min_score, 1))
    return sorted(zip(i.tolist(), j.tolist(), S[i, j].tolist()), key=lambda t: (-t[2], t[0], t[1]))  # -0.0 == 0.0 in Python too


def check(idx, ids, S, min_score, metric=COS, limit=None, route="mfma", handed=0):
    exp = expected(S, min_score)
    a, b, s, total = idx.similarity_join_arrays(min_score, metric, limit)
    lj = idx.last_join()
    want = exp if limit is None else exp[:limit]
    assert total == len(exp), (min_score, total, len(exp), lj)
    assert a.tolist() == [int(ids[i]) for i, _, _ in want] and b.tolist() == [int(ids[j]) for _, j, _ in want], (min_score, lj)
    assert bits(s) == bits([x for _, _, x in want]), (min_score, lj)
    assert lj["qualifying_pairs"] == total
    if len(ids) >= 2:
        assert lj["route"] == route and (route != "mfma" or lj["panels_handed_back"] == handed), lj
    return lj


def make(V, dim, rows, seed=0):
    # ids carry no order and repeat: duplicate ids are distinct rows
    ids = np.random.default_rng(seed).permutation(len(rows)).astype(np.uint64) * np.uint64(7) % np.uint64(max(len(rows) - 1, 1))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    return idx, ids


@pytest.mark.parametrize("n,dim", [(1, 384), (2, 384), (33, 384), (129, 384), (274, 384), (700, 384), (274, 100), (274, 768)])
def test_mfma_route_matches_brute_force(V, O, n, dim):
    rows, pairs = planted_rows(n, dim, 100 * n + dim)
    idx, ids = make(V, dim, rows)
    S = pair_scores(O, rows, COS)
    lj = check(idx, ids, S, 0.8)
    if n >= 2:
        assert lj["candidate_pairs"] >= lj["qualifying_pairs"] >= 1 and lj["candidate_pairs"] < 200, lj
        tie = float(S[pairs[0]])  # on a planted pair's score the pair is in; on its f64 successor it is out
        t_in = check(idx, ids, S, tie)["qualifying_pairs"]
        t_out = check(idx, ids, S, float(np.nextafter(tie, np.inf)))["qualifying_pairs"]
        assert t_in > t_out
        # capacity: a prefix of the full order with the exact total; 0 counts
        check(idx, ids, S, 0.75, limit=2)
        check(idx, ids, S, 0.75, limit=0)


@pytest.mark.parametrize("dim", [128, 384, 768])
def test_pair_on_the_edge_of_the_bf16_slack(V, O, dim):
    # parallel rows whose unit components sit just under a bf16 rounding boundary (section 17's construction): the key loses
    # 0.00775 of a score of 1, the bound allows 0.0079 -- the pair must be a candidate with min_score ON its score
    e = 2.0 ** np.array([-1] * 3 + [-2] * 3 + [-3] * 3 + [-4] * 2 + [-7], dtype=np.float64)
    assert float((e * e).sum()) == 127.0 / 128.0 + 2.0 ** -14
    rows = np.random.default_rng(dim).standard_normal((40, dim))
    rows[7] = 0.0
    rows[7, dim - e.size:] = 2.5 * e
    rows[21] = rows[7] * 0.28
    idx, ids = make(V, dim, rows)
    S = pair_scores(O, rows, COS)
    lj = check(idx, ids, S, float(S[7, 21]))
    assert lj["qualifying_pairs"] >= 1 and S[7, 21] >= 1.0 - 1e-15


def test_candidate_overflow_splits_ranges_and_hands_panels_back(V, O, monkeypatch):
    rows, _ = planted_rows(700, 384, 7)
    rows[300:340] = rows[300] * np.linspace(0.5, 2.0, 40)[:, None]  # 780 pairs inside panel 2
    rows[600:630] = rows[600] * np.linspace(0.5, 2.0, 30)[:, None]  # 435 pairs inside panel 4
    idx, ids = make(V, 384, rows)
    S = pair_scores(O, rows, COS)
    free = check(idx, ids, S, 0.8)
    assert free["launches"] == 1
    monkeypatch.setenv("VL_JOIN_CAND_CAP", "800")  # the whole range overflows, its halves hold
    split = check(idx, ids, S, 0.8)
    assert split["launches"] > 1 and split["panels_answered"] == free["panels_answered"], split
    monkeypatch.setenv("VL_JOIN_CAND_CAP", "100")  # panels 2 and 4 overflow on their own: the loop answers their rows
    back = check(idx, ids, S, 0.8, handed=2)
    assert back["panels_answered"] == free["panels_answered"] - 2, back
    check(idx, ids, S, 0.8, limit=5, handed=2)


def test_after_delete_update_and_add(V, O):
    rows, _ = planted_rows(274, 384, 11)
    ids = np.arange(1000, 1274, dtype=np.uint64)  # unique ids: delete and update name rows by id
    idx = V.FlatIndex(384)
    idx.add_rows(ids, rows, validate=False)
    idx.similarity_join_arrays(0.8)  # builds the lazy bf16 copy
    idx.delete(int(ids[9]))
    rows = np.delete(rows, 9, axis=0)
    ids = np.delete(ids, 9)
    rows[100] = rows[200] * 1.5
    idx.update_rows(ids[100:101], rows[100:101])
    extra = rows[[0, 50]] * 0.5
    idx.add_rows(np.array([5000, 5001], dtype=np.uint64), extra, validate=False)
    rows, ids = np.vstack([rows, extra]), np.concatenate([ids, [5000, 5001]])
    check(idx, ids, pair_scores(O, rows, COS), 0.8)


@pytest.mark.parametrize("metric,min_score", [(EUC, 0.06), (MAN, 0.0041), (DOT, 300.0), (COS, float("-inf"))])
def test_loop_route(V, O, metric, min_score):
    rows, _ = planted_rows(129, 384, 13)
    idx, ids = make(V, 384, rows)
    if metric == MAN:
        idx.set_join_route("mfma")  # an ineligible call takes the loop and says so
    S = pair_scores(O, rows, metric)
    lj = check(idx, ids, S, min_score, metric, route="loop")
    assert lj["qualifying_pairs"] >= 3
    check(idx, ids, S, min_score, metric, limit=2, route="loop")


def test_forced_loop_equals_mfma_and_refusals(V, O):
    rows, _ = planted_rows(274, 384, 17)
    idx, ids = make(V, 384, rows)
    S = pair_scores(O, rows, COS)
    idx.set_join_route("loop")
    check(idx, ids, S, 0.8, route="loop")
    with pytest.raises(V.IndexOpError, match="NaN"):
        idx.similarity_join_arrays(float("nan"))
    h = V.HNSWIndex(384)
    for call in (lambda: h.similarity_join_arrays(0.8), lambda: h.set_join_route("loop"), h.last_join):
        with pytest.raises(V.IndexOpError, match="single-GPU flat"):
            call()
