"""Late-interaction (MaxSim) search (vl_index_search_maxsim) against the definition: the oracle's
FlatOracle.search(q_t, n, metric) per token, the max per group, a Python float sum in token order, sorted by (-score, key).
Group keys and score bits are compared.  The MFMA cases demand the MFMA route: before they do, they compute in numpy how
many groups a bound with a slack of 0.0085 per token (rows and tokens are about unit length) cannot rule out, and require
that number below the cap -- a case the exact route answered says nothing about the kernel."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, EUC, MAN, DOT = 0, 1, 2, 3
CAND_CAP = 4096  # MAXSIM_CAND_CAP


@pytest.fixture(scope="module")
def V():
    import vectorlite_amd as V
    n_dev, _ = V.runtime_info()
    assert n_dev > 0, "GPU tests need a HIP device"
    return V


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64).tolist()


def group_of_rows(n, layout):
    """Dense group number per row, -1 = no group.  runN: runs of N consecutive rows (5 and 40 cross the 16- and 32-row block
    edges); robin: rows dealt round-robin to 50 groups (every block mixed); third: runs of 5 with every third run ungrouped."""
    p = np.arange(n)
    if layout == "robin":
        return p % 50
    if layout == "third":
        return np.where((p // 5) % 3 == 1, -1, p // 5)
    return p // int(layout[3:])


@functools.lru_cache(maxsize=4)
def data(dim, n, layout, n_tokens, noise=0.1):
    """Unit rows, their groups, keys that are NOT in group order, and tokens that are noisy copies of rows of three target
    groups (noise = None: i.i.d. gaussian tokens), so that those groups stand clear of the rest."""
    rng = np.random.default_rng(1000 * dim + n + 7 * n_tokens + len(layout))
    rows = rng.standard_normal((n, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    gor = group_of_rows(n, layout)
    n_groups = int(gor.max()) + 1
    keys = (np.arange(n_groups, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 40) + np.uint64(5)
    if noise is None:
        Q = rng.standard_normal((n_tokens, dim)) / np.sqrt(dim)
    else:
        targets = rng.choice(np.unique(gor[gor >= 0]), size=min(3, n_groups), replace=False)
        src = [rng.choice(np.nonzero(gor == targets[t % len(targets)])[0]) for t in range(n_tokens)]
        Q = rows[src] + noise * rng.standard_normal((n_tokens, dim)) / np.sqrt(dim)
    return rows, gor, keys, np.ascontiguousarray(Q)


@functools.lru_cache(maxsize=4)
def reference(dim, n, layout, n_tokens, metric, noise=0.1):
    """[(key, score)] of every group with a row, best first, from the oracle's per-token scores."""
    from oracle import oracle as O
    rows, gor, keys, Q = data(dim, n, layout, n_tokens, noise)
    ref = O.FlatOracle(dim, np.arange(n, dtype=np.uint64), rows)
    groups = sorted(set(gor[gor >= 0].tolist()))
    members = [np.nonzero(gor == g)[0] for g in groups]
    best = []
    for q in Q:
        ri, rs = ref.search(q, n, metric)
        s = np.empty(n)
        s[ri.astype(np.int64)] = rs
        best.append([max(s[m].tolist()) for m in members])
    scored = [(int(keys[g]), sum(best[t][i] for t in range(n_tokens))) for i, g in enumerate(groups)]
    return sorted(scored, key=lambda e: (-e[1], e[0]))


_built = {}


def build(V, dim, n, layout, n_tokens, noise=0.1):
    """One index and group table per data set (ids = 10 * position + 1), kept for the k and metric cases that share it."""
    key = (dim, n, layout, n_tokens, noise)
    if key not in _built:
        _built.clear()
        rows, gor, keys, _ = data(*key)
        idx = V.FlatIndex(dim)
        ids = np.arange(n, dtype=np.uint64) * np.uint64(10) + np.uint64(1)
        idx.add_rows(ids, rows, validate=False)
        _built[key] = (idx, idx.make_groups(ids[gor >= 0], keys[gor[gor >= 0]]))
    return _built[key]


def check(idx, groups, Q, k, metric, exp, route=None):
    gk, gs = idx.search_maxsim_arrays(Q, k, metric, groups=groups)
    lm = idx.last_maxsim()
    want = exp[:k]
    assert gk.tolist() == [e[0] for e in want], lm
    assert bits(gs) == bits([e[1] for e in want]), lm
    if route is not None:
        assert lm["route"] == route, lm
    return lm


# every dim, row count, layout, token count (1, 2, 17, 96 | 97, 128: one and two chunks at stride 768) and metric at least once
CASES = [(100, 33, "run1", 1, COS), (128, 33, "run5", 2, EUC), (384, 33, "robin", 17, DOT), (768, 33, "run16", 97, COS),
         (100, 4133, "run40", 17, EUC), (128, 4133, "run16", 128, COS), (384, 4133, "run5", 96, DOT), (384, 4133, "robin", 2, COS),
         (768, 4133, "run40", 96, EUC), (768, 4133, "third", 128, DOT), (768, 4133, "run1", 97, COS), (128, 4133, "third", 1, EUC),
         (384, 4133, "run1", 17, EUC), (100, 4133, "robin", 128, DOT)]


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("dim,n,layout,n_tokens,metric", CASES)
def test_mfma_route_matches_the_definition(V, dim, n, layout, n_tokens, metric, k):
    exp = reference(dim, n, layout, n_tokens, metric)
    L = exp[min(k, len(exp)) - 1][1]
    cannot_rule_out = sum(1 for _, s in exp if s + n_tokens * 0.0085 >= L)
    assert cannot_rule_out <= CAND_CAP, "the data alone must keep the survivors below the cap"
    idx, groups = build(V, dim, n, layout, n_tokens)
    lm = check(idx, groups, data(dim, n, layout, n_tokens)[3], k, metric, exp, route="mfma")
    assert min(k, len(exp)) <= lm["survivors"] <= CAND_CAP and lm["member_rows"] >= lm["survivors"], lm
    assert lm["chunks"] == (2 if dim == 768 and n_tokens > 96 else 1), lm
    assert V.last_path() == V.PATH_FAST


@pytest.mark.parametrize("metric,k", [(MAN, 10), (COS, 65), (DOT, 1000)])
def test_exact_route_for_manhattan_and_large_k(V, metric, k):
    shape = (100, 4133, "run5", 2)
    idx, groups = build(V, *shape)
    check(idx, groups, data(*shape)[3], k, metric, reference(*shape, metric), route="exact")
    assert V.last_path() == V.PATH_EXACT_SORT


def test_forced_exact_path_equals_the_fast_answer(V):
    shape = (384, 4133, "run5", 96)
    idx, groups = build(V, *shape)
    Q = data(*shape)[3]
    fast = idx.search_maxsim_arrays(Q, 64, EUC, groups=groups)
    assert idx.last_maxsim()["route"] == "mfma"
    idx.force_path(V.PATH_EXACT_SORT)
    try:
        forced = idx.search_maxsim_arrays(Q, 64, EUC, groups=groups)
        assert idx.last_maxsim()["route"] == "exact"
    finally:
        idx.force_path(V.PATH_NONE)
    assert fast[0].tolist() == forced[0].tolist() and bits(fast[1]) == bits(forced[1])


def test_identical_groups_come_out_in_key_order_and_the_token_survives_delete_and_add(V):
    rows, gor, keys, Q = (a.copy() for a in data(128, 33, "run5", 2))
    rows[10:15] = rows[0:5]  # groups 0 and 2 hold the same rows; the tokens are copies of rows of three other groups or these
    Q[0] = rows[2]
    Q[1] = rows[3]
    keys[0], keys[2] = 900, 800
    ids = np.arange(33, dtype=np.uint64) + np.uint64(100)
    idx = V.FlatIndex(128)
    idx.add_rows(ids, rows, validate=False)
    groups = idx.make_groups(ids, keys[gor])
    for metric in (COS, EUC, DOT, MAN):
        gk, gs = idx.search_maxsim_arrays(Q, 3, metric, groups=groups)
        assert gk.tolist()[:2] == [800, 900] and bits(gs[:1]) == bits(gs[1:2]), (metric, gk, gs)
    # the token follows the index: group 2 loses its rows, a new row joins group 0 under an id the table already holds
    for i in range(110, 115):
        idx.delete(int(i))
    gk, _ = idx.search_maxsim_arrays(Q, 10, COS, groups=groups)
    assert gk.tolist()[0] == 900 and 800 not in gk.tolist() and len(gk) == 6
    idx.add_rows(np.array([112], dtype=np.uint64), rows[12:13], validate=False)
    gk, gs = idx.search_maxsim_arrays(Q, 10, COS, groups=groups)  # group 2 matches token 0 as well as group 0, token 1 less well
    assert gk.tolist()[:2] == [900, 800] and len(gk) == 7 and idx.last_maxsim()["route"] == "mfma"


def test_survivors_above_the_cap_go_to_the_exact_route(V, monkeypatch):
    shape = (128, 4133, "run1", 17, None)  # i.i.d. gaussian tokens: no group stands clear
    idx, groups = build(V, *shape)
    monkeypatch.setenv("VL_MAXSIM_CAND_CAP", "16")
    lm = check(idx, groups, data(*shape)[3], 10, COS, reference(*shape[:4], COS, None), route="exact")
    assert lm["survivors"] > 16, lm


def test_nan_row_fails_only_inside_a_group_and_argument_errors(V):
    rows, gor, keys, Q = data(128, 33, "run5", 2)
    rows = rows.copy()
    rows[32, 5] = np.nan  # row 32 is the last group's
    ids = np.arange(33, dtype=np.uint64)
    idx = V.FlatIndex(128)
    idx.add_rows(ids, rows, validate=False)
    with_nan = idx.make_groups(ids, keys[gor])
    without = idx.make_groups(ids[:30], keys[gor[:30]])
    with pytest.raises(V.NaNScore):
        idx.search_maxsim_arrays(Q, 3, COS, groups=with_nan)
    gk, _ = idx.search_maxsim_arrays(Q, 3, COS, groups=without)
    assert len(gk) == 3 and idx.last_maxsim()["route"] == "exact"
    for bad_q in (np.zeros((0, 128)), np.zeros((129, 128))):
        with pytest.raises(V.IndexOpError):
            idx.search_maxsim_arrays(bad_q, 3, COS, groups=without)
    with pytest.raises(V.IndexOpError):
        idx.search_maxsim_arrays(Q, 3, 7, groups=without)
    with pytest.raises(V.IndexOpError):
        idx.search_maxsim_arrays(Q, 1025, COS, groups=without)
    without.close()
    with pytest.raises(V.IndexOpError):
        idx.search_maxsim_arrays(Q, 3, COS, groups=without)
    with pytest.raises(V.DimensionMismatch):
        idx.search_maxsim_arrays(Q[:, :100], 3, COS, groups=with_nan)
