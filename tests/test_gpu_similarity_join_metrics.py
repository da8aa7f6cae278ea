"""The Euclidean and dot-product similarity joins on the MFMA pass (route "mfma") against brute force
over the oracle's pair scores, with test_gpu_similarity_join.py's method: ids, score bits, total and the route.  Rows have
gaussian directions and lengths spread over 0.25 .. 4, so the per-pair slack of the threshold is exercised.

The candidate cap n (n - 1) / 8 is asserted from n = 33 up: at n = 2 it is 0.25 and contradicts candidates >= qualifying = 1."""
import numpy as np
import pytest

from test_gpu_similarity_join import O, V, bits, expected, pair_scores  # noqa: F401 (V and O are fixtures)

pytestmark = pytest.mark.gpu

EUC, DOT = 1, 3
SHAPES = [(2, 384), (33, 384), (129, 384), (274, 384), (274, 100), (274, 768)]


def rows_of_mixed_length(n, dim, seed):
    """Near-duplicates (perturbed by 2 % of the row, rows 3.2 .. 4 long so that their dot products stand out too) inside a
    16-row group, across a 32-row block edge, across the 128- and 96-row panel edges, first and last row, the partial last
    block; rows 5, 6, 7 identical; row 12 zero; rows 20, 21 differ only in length."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, dim))
    rows *= (np.exp(rng.uniform(np.log(0.25), np.log(4.0), n)) / np.linalg.norm(rows, axis=1))[:, None]
    rows[0] *= 0.25 / np.linalg.norm(rows[0])  # the spread reaches both ends
    if n > 1:
        rows[1] *= 4.0 / np.linalg.norm(rows[1])
    planted = []
    for a, b in [(0, n - 1), (3, 9), (31, 32), (127, 128), (95, 96), (5, 6), (5, 7), (n - 3, n - 2), (20, 21)]:
        if not (0 <= a < b < n) or any(b in p for p in planted) or (a != 5 and any(a in p for p in planted)):
            continue
        if a != 5 or b == 6:
            rows[a] *= rng.uniform(3.2, 4.0) / np.linalg.norm(rows[a])
        w = rng.standard_normal(dim)
        rows[b] = rows[a] if a == 5 else (rows[a] * 1.02 if a == 20 else rows[a] + 0.02 * np.linalg.norm(rows[a]) * w / np.linalg.norm(w))
        planted.append((a, b))
    if n > 12:
        rows[12] = 0.0
    return rows, planted


def reference_candidates(rows, metric, min_score):
    """Pairs whose exact cosine is at least (the cosine min_score implies for the pair's lengths) - 0.02."""
    nrm = np.linalg.norm(rows, axis=1)
    p = np.outer(nrm, nrm)
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = np.where(p > 0, (rows @ rows.T) / p, 0.0)
        sq = nrm[:, None] ** 2 + nrm[None, :] ** 2
        d2 = (1.0 / min_score - 1.0) ** 2
        implied = np.where(p > 0, min_score / p if metric == DOT else (sq - d2) / (2 * p), np.inf)
    with_zero_row = (p == 0) & ((min_score <= 0) if metric == DOT else (sq <= d2))  # no cosine: the score decides
    return int(np.triu((cos >= implied - 0.02) | with_zero_row, 1).sum())


def make(V, dim, rows, ids=None):
    ids = np.arange(len(rows), dtype=np.uint64) * np.uint64(7) % np.uint64(max(len(rows) - 1, 1)) if ids is None else ids  # ids repeat
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    idx.set_join_route("mfma")
    return idx, ids


def check(idx, ids, S, min_score, metric, limit=None, route="mfma"):
    exp = expected(S, min_score)
    a, b, s, total = idx.similarity_join_arrays(min_score, metric, limit)
    lj = idx.last_join()
    want = exp if limit is None else exp[:limit]
    assert lj["route"] == route, lj
    assert total == len(exp) == lj["qualifying_pairs"], (min_score, total, len(exp), lj)
    assert a.tolist() == [int(ids[i]) for i, _, _ in want] and b.tolist() == [int(ids[j]) for _, j, _ in want], (min_score, lj)
    assert bits(s) == bits([x for _, _, x in want]), (min_score, lj)
    return lj


def tie_score(S, planted):
    return min(float(S[p]) for p in planted)  # every planted pair qualifies on it


@pytest.mark.parametrize("metric", [EUC, DOT])
@pytest.mark.parametrize("n,dim", SHAPES)
def test_mfma_route_matches_brute_force(V, O, metric, n, dim):
    rows, planted = rows_of_mixed_length(n, dim, 100 * n + dim)
    idx, ids = make(V, dim, rows)
    S = pair_scores(O, rows, metric)
    tie = tie_score(S, planted)
    lj = check(idx, ids, S, tie, metric)
    assert lj["panels_handed_back"] == 0 and lj["qualifying_pairs"] >= min(3, len(planted)), lj
    assert lj["candidate_pairs"] >= lj["qualifying_pairs"], lj
    if n > 2:
        cap = n * (n - 1) / 8
        assert reference_candidates(rows, metric, tie) <= cap, "the planted scores alone must satisfy the cap"
        assert lj["candidate_pairs"] <= cap, lj
    out = check(idx, ids, S, float(np.nextafter(tie, np.inf)), metric)  # on the f64 successor the pair is out
    assert out["qualifying_pairs"] < lj["qualifying_pairs"]
    check(idx, ids, S, tie, metric, limit=2)
    check(idx, ids, S, tie, metric, limit=0)


@pytest.mark.parametrize("metric", [EUC, DOT])
def test_small_buffer_then_delete_and_add_then_auto(V, O, metric, monkeypatch):
    rows, planted = rows_of_mixed_length(274, 384, 7)
    idx, ids = make(V, 384, rows, np.arange(1000, 1274, dtype=np.uint64))
    S = pair_scores(O, rows, metric)
    tie = tie_score(S, planted)
    monkeypatch.setenv("VL_JOIN_CAND_CAP", "2")  # panel 0 alone holds six planted pairs: the loop answers its rows
    lj = check(idx, ids, S, tie, metric)
    assert lj["launches"] > 1 and lj["panels_handed_back"] >= 1 and lj["panels_answered"] >= 1, lj
    monkeypatch.delenv("VL_JOIN_CAND_CAP")
    idx.delete(int(ids[9]))
    rows, ids = np.delete(rows, 9, axis=0), np.delete(ids, 9)
    extra = rows[[1, 50]] * 1.01
    idx.add_rows(np.array([5000, 5001], dtype=np.uint64), extra, validate=False)
    rows, ids = np.vstack([rows, extra]), np.concatenate([ids, [5000, 5001]])
    S = pair_scores(O, rows, metric)
    assert check(idx, ids, S, tie, metric)["panels_handed_back"] == 0
    idx.set_join_route("auto")  # not measured: auto keeps the two metrics on the loop
    check(idx, ids, S, tie, metric, route="loop")
