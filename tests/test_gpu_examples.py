"""Search by positive and negative examples (vl_index_search_examples) against the definition: the
oracle's FlatOracle.search(example, n, metric) gives every row's score per example; P, N and f are formed as Python floats
(the maxima with -0.0 below +0.0, the strict P > N, one multiply and a negation), sorted by (-f, position).  Ids and score
bits are compared.  The MFMA cases demand the MFMA route: 4133 rows are below the survivor cap (8192), so the data cannot
push them off it.  Run as a program it prints one call's answer as JSON (the cap-overflow case's fresh child process)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


@functools.lru_cache(maxsize=2)
def stored(dim, n):
    """Rows of norm 0.5 .. 2 (dot and Euclidean read the norm) and their ids (10 * position + 1)."""
    rng = np.random.default_rng(33 * dim + n)
    rows = rng.standard_normal((n, dim))
    rows *= (rng.uniform(0.5, 2.0, n) / np.linalg.norm(rows, axis=1))[:, None]
    return rows, np.arange(n, dtype=np.uint64) * np.uint64(10) + np.uint64(1)


@functools.lru_cache(maxsize=4)
def examples(dim, n, a, b):
    """Positives: noisy copies of stored rows; negatives: noisy copies of other rows; norms spread over 0.3 .. 3."""
    rows, _ = stored(dim, n)
    rng = np.random.default_rng(1000 * dim + n + 7 * a + b)
    src = rng.choice(n, size=a + b, replace=a + b > n)
    E = rows[src] / np.linalg.norm(rows[src], axis=1, keepdims=True) + 0.1 * rng.standard_normal((a + b, dim)) / np.sqrt(dim)
    E *= np.geomspace(0.3, 3.0, a + b)[rng.permutation(a + b)][:, None]
    return np.ascontiguousarray(E[:a]), np.ascontiguousarray(E[a:])


def ordered_max(S):
    """Column maxima of S [examples, rows] with -0.0 below +0.0."""
    m = S.max(axis=0)
    plus = ((S == 0) & ~np.signbit(S)).any(axis=0)
    return np.where(m == 0, np.where(plus, 0.0, -0.0), m)


def reference(rows, pos, neg, metric):
    """[(position, f)] of every row, best first."""
    from oracle import oracle as O
    n = len(rows)
    ref = O.FlatOracle(rows.shape[1], np.arange(n, dtype=np.uint64), rows)

    def side(E):
        S = np.empty((len(E), n))
        for e, q in enumerate(E):
            ri, rs = ref.search(q, n, metric)
            S[e, ri.astype(np.int64)] = rs
        return ordered_max(S).tolist()
    P = side(pos)
    f = P if len(neg) == 0 else [p if p > m else -(m * m) for p, m in zip(P, side(neg))]
    return sorted(enumerate(f), key=lambda e: (-e[1], e[0]))


@functools.lru_cache(maxsize=4)
def case_reference(dim, n, a, b, metric):
    return reference(stored(dim, n)[0], *examples(dim, n, a, b), metric)


_built = {}


def build(V, dim, n):
    """One index per stored data set, kept for the cases that share it."""
    if (dim, n) not in _built:
        _built.clear()
        rows, ids = stored(dim, n)
        idx = V.FlatIndex(dim)
        idx.add_rows(ids, rows, validate=False)
        _built[(dim, n)] = idx
    return _built[(dim, n)]


def check(idx, pos, neg, k, metric, exp, route=None):
    ids, fs = idx.search_examples_arrays(pos, neg if len(neg) else None, k, metric)
    le = idx.last_examples()
    want = exp[:k]
    assert ids.tolist() == [10 * p + 1 for p, _ in want], le
    assert bits(fs) == bits([f for _, f in want]), le
    if route is not None:
        assert le["route"] == route, le
    return le


# every stride (dims 100 / 128 -> 128, 200 -> 256, 384, 512, 768) with cosine, Euclidean and dot; 33 rows (a partial 32-row
# block) and 4133 (more blocks than one workgroup's waves per CU); (a, b): a lone block, a block boundary on each side, a
# ragged last block, all six blocks
CASES = [(100, 33, 1, 0, COS), (128, 33, 2, 1, EUC), (100, 4133, 17, 3, DOT), (128, 4133, 64, 32, COS),
         (200, 33, 17, 3, COS), (200, 33, 1, 0, DOT), (200, 4133, 2, 1, EUC),
         (384, 33, 16, 16, DOT), (384, 4133, 1, 0, EUC), (384, 4133, 16, 16, COS),
         (512, 33, 17, 3, COS), (512, 4133, 2, 1, DOT), (512, 4133, 64, 32, EUC),
         (768, 33, 64, 32, EUC), (768, 4133, 16, 16, DOT), (768, 4133, 17, 3, COS)]


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("dim,n,a,b,metric", CASES)
def test_mfma_route_matches_the_definition(V, dim, n, a, b, metric, k):
    exp = case_reference(dim, n, a, b, metric)
    le = check(build(V, dim, n), *examples(dim, n, a, b), k, metric, exp, route="mfma")
    assert le["seeds"] == min(n, 64) and min(k, n) <= le["survivors"] <= n, le
    assert le["blocks"] == (a + 15) // 16 + (b + 15) // 16, le
    assert V.last_path() == V.PATH_FAST


@pytest.mark.parametrize("metric", [COS, EUC, DOT, MAN])
def test_strict_rule_scores_a_shared_example_by_its_negative_and_duplicates_tie_by_position(V, metric):
    rows, _ = (x.copy() for x in stored(128, 33))
    pos, neg = (x.copy() for x in examples(128, 33, 2, 1))
    rows[5] = rows[20] = neg[0] = pos[0]  # one vector in both lists and twice in the index: P == N there, so f = -(N N)
    idx = V.FlatIndex(128)
    idx.add_rows(np.arange(33, dtype=np.uint64) * np.uint64(10) + np.uint64(1), rows, validate=False)
    exp = reference(rows, pos, neg, metric)
    check(idx, pos, neg, 33, metric, exp, route="exact" if metric == MAN else "mfma")
    f = dict(exp)
    order = [p for p, _ in exp]
    assert f[5] < 0 and bits([f[5]]) == bits([f[20]]) and order.index(20) == order.index(5) + 1


def test_dominating_negatives_make_every_row_a_survivor(V):
    dim, n = 384, 4133
    pos, _ = examples(dim, n, 8, 0)
    neg = np.concatenate([pos, stored(dim, n)[0][:8]])  # the positives themselves among the negatives: P <= N everywhere
    exp = reference(stored(dim, n)[0], pos, neg, COS)
    assert exp[0][1] <= 0
    le = check(build(V, dim, n), pos, neg, 10, COS, exp, route="mfma")
    assert le["survivors"] == n, le


@pytest.mark.parametrize("metric,k", [(MAN, 10), (COS, 65), (DOT, 1000)])
def test_exact_route_for_manhattan_and_large_k(V, metric, k):
    shape = (100, 4133, 17, 3)
    check(build(V, *shape[:2]), *examples(*shape), k, metric, case_reference(*shape, metric), route="exact")
    assert V.last_path() == V.PATH_EXACT_SORT


def test_forced_exact_path_equals_the_fast_answer(V):
    shape = (384, 4133, 16, 16)
    idx = build(V, *shape[:2])
    pos, neg = examples(*shape)
    fast = idx.search_examples_arrays(pos, neg, 64, EUC)
    assert idx.last_examples()["route"] == "mfma"
    idx.force_path(V.PATH_EXACT_SORT)
    try:
        forced = idx.search_examples_arrays(pos, neg, 64, EUC)
        assert idx.last_examples()["route"] == "exact"
    finally:
        idx.force_path(V.PATH_NONE)
    assert fast[0].tolist() == forced[0].tolist() and bits(fast[1]) == bits(forced[1])


def test_survivors_above_the_cap_go_to_the_exact_route_in_a_fresh_process():
    shape = (128, 4133, 17, 3)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *map(str, shape), str(COS), "10"], capture_output=True, text=True,
                       env=dict(os.environ, VL_EXAMPLES_CAND_CAP="5"), timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = json.loads(r.stdout.strip().splitlines()[-1])
    want = case_reference(*shape, COS)[:10]
    assert got["last"]["route"] == "exact" and got["last"]["survivors"] > 5, got
    assert got["ids"] == [10 * p + 1 for p, _ in want] and got["bits"] == bits([f for _, f in want])


def test_nan_row_and_argument_rules(V):
    rows, ids = (x.copy() for x in stored(128, 33))
    pos, neg = examples(128, 33, 2, 1)
    idx = V.FlatIndex(128)
    assert len(idx.search_examples_arrays(pos, neg, 3, COS)[0]) == 0  # an empty index
    idx.add_rows(ids, rows, validate=False)
    assert len(idx.search_examples_arrays(pos, neg, 0, COS)[0]) == 0  # k = 0
    for bad_pos, bad_neg in ((np.zeros((0, 128)), None), (np.zeros((65, 128)), None), (pos, np.zeros((33, 128)))):
        with pytest.raises(V.IndexOpError):
            idx.search_examples_arrays(bad_pos, bad_neg, 3, COS)
    with pytest.raises(V.IndexOpError):
        idx.search_examples_arrays(pos, neg, 3, 7)
    with pytest.raises(V.DimensionMismatch):
        idx.search_examples_arrays(pos[:, :100], neg[:, :100], 3, COS)
    rows[32, 5] = np.nan
    bad = V.FlatIndex(128)
    bad.add_rows(ids, rows, validate=False)
    with pytest.raises(V.NaNScore):
        bad.search_examples_arrays(pos, neg, 3, COS)
    assert bad.last_examples()["route"] != "mfma"
    hnsw = V.HNSWIndex(128)
    n_out = C.c_uint64(7)
    assert hnsw._L.vl_index_search_examples(hnsw._h, pos.ctypes.data, 2, None, 0, 128, 3, COS, 0, None, None,
                                            C.byref(n_out)) == V.VL_ERR_INVALID_ARG and n_out.value == 0


if __name__ == "__main__":  # dim n a b metric k -> {"ids", "bits", "last"} of one call, for the cap-overflow case's child
    sys.path.insert(0, ROOT)
    import vectorlite_amd as V
    dim, n, a, b, metric, k = map(int, sys.argv[1:7])
    rows, ids = stored(dim, n)
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    pos, neg = examples(dim, n, a, b)
    got_ids, got_f = idx.search_examples_arrays(pos, neg if b else None, k, metric)
    print(json.dumps({"ids": got_ids.tolist(), "bits": bits(got_f), "last": idx.last_examples()}))
