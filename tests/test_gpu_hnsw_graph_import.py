"""HNSW graph import (vl_index_hnsw_graph_import, HNSWIndex.from_graph / save_snapshot / load_snapshot; DESIGN.md
"Importing a graph").

1. Round trip: an index imported from another's export has the same export, answers every search with the same ids and
   score bits in both navigations with the same number of distance evaluations, and goes on living (clone, delete, add).
2. A graph no GPU build made (brute-force lists of every length 0 .. m0, an empty list, a node nobody names): orphans are
   reported, the reference navigation equals the CPU walker node for node, and a full-beam f32 walk returns exactly the
   layer-0 reachable set of its landing point in exact order.
3. Refusals: each leaves the handle empty and usable.  The lists are validated on the host, so no device kernel ever sees
   one of these.
4. Snapshots.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
METRICS = (0, 1, 2, 3)  # cosine, euclidean, manhattan, dot
NQ = 16
ARRAYS = ("level", "upper_off", "cnt0", "nbr0", "cntU", "nbrU", "node_ids", "live", "rows")


@pytest.fixture(scope="module")
def VO():
    import vectorlite_amd as V
    from oracle import oracle as O
    O.build()
    return V, O


def _ids(n):
    return np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(3)


def _same_graph(ga, gb):
    assert (ga["n"], ga["entry"], ga["max_level"], ga["m"], ga["m0"]) == (gb["n"], gb["entry"], gb["max_level"], gb["m"], gb["m0"])
    for key in ARRAYS:
        assert ga[key].dtype == gb[key].dtype and ga[key].shape == gb[key].shape, key
        assert ga[key].tobytes() == gb[key].tobytes(), key


def _answers(idx, Q, metric, n):
    """Every (navigation, k, ef) cell as bytes, and the distance evaluations the whole sweep made."""
    out = []
    e0 = idx.walk_stats()[1]
    for mode in ("f32", "reference"):
        idx.set_navigation(mode)
        for k in sorted({1, min(10, n), n}):
            for ef in (0, 10, 64, 512):
                ids, scores, cnt = idx.search_batch(Q, k, metric, ef=ef)
                rows = [(ids[i, :int(cnt[i])].tobytes(), scores[i, :int(cnt[i])].tobytes()) for i in range(len(Q))]
                out.append((mode, k, ef, cnt.tolist(), rows))
    idx.set_navigation("f32")
    return out, idx.walk_stats()[1] - e0


def _round_trip(V, metric, n, dim, m=16, m0=32):
    rng = np.random.default_rng(7000 + 100 * metric + n + dim + m)
    X, Q, ids = rng.standard_normal((n, dim)), rng.standard_normal((NQ, dim)), _ids(n)
    A = V.HNSWIndex(dim, metric, m=m, m0=m0, seed=5)
    A.add_rows(ids, X)
    dead = []
    if n >= 33:
        entry = A.graph()["entry"]
        dead = sorted(([entry] + [v for v in (0, 1, n // 2, n - 2, n - 1) if v != entry])[:5])  # five, the entry point among them
        for v in dead:
            A.delete(int(ids[v]))
    ga, p = A.graph(with_rows=True), A.params()
    assert p == {"m": m, "m0": m0, "ef_construction": 400, "seed": 5}
    B = V.HNSWIndex.from_graph(ga, dim, metric, **p)
    assert B._meta == {} and B.params() == p
    _same_graph(ga, B.graph(with_rows=True))
    assert ga["live"].sum() == n - len(dead)
    assert ga["level"].tolist() == [V.hnsw_level(5, i, m) for i in range(n)]

    ans_a, evals_a = _answers(A, Q, metric, n)
    ans_b, evals_b = _answers(B, Q, metric, n)
    assert ans_a == ans_b
    assert evals_a == evals_b and evals_a > 0
    assert any(c for _, _, _, cnt, _ in ans_a for c in cnt)  # nothing passes vacuously

    assert B.len() == A.len() == n - len(dead) and B.max_id() == A.max_id()
    ea, eb = A.export(), B.export()
    assert ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes()
    for v in (0, n // 2, n - 1):
        va, vb = A.get_vector(int(ids[v])), B.get_vector(int(ids[v]))
        assert (va is None) == (vb is None) == (v in dead)
        if va is not None:
            assert np.asarray(va.values).tobytes() == np.asarray(vb.values).tobytes() == X[v].tobytes()
    C = B.clone()
    _same_graph(ga, C.graph(with_rows=True))
    assert _answers(C, Q, metric, n)[0] == ans_a
    # the imported index goes on living: the build's link phase reads the recomputed edge keys and in-degrees
    live_before = B.len()
    if n >= 33:
        B.delete(int(ids[next(v for v in range(n) if v not in dead)]))
        live_before -= 1
    extra = rng.standard_normal((50, dim))
    B.add_rows(np.arange(50, dtype=np.uint64) + np.uint64(10 ** 6), extra)
    assert B.len() == live_before + 50 and B.graph()["n"] == n + 50
    got, _, cnt = B.search_batch(extra[:4], 1, metric, ef=64)
    assert (cnt == 1).all()
    if metric in (1, 2):  # a row is its own nearest neighbour under the two true distances
        assert got[:, 0].tolist() == [10 ** 6 + i for i in range(4)]
    assert A.len() == n - len(dead)  # the source is untouched


@pytest.mark.parametrize("n,dim", ((1, 3), (2, 3), (33, 7), (1100, 16), (3000, 384)))
@pytest.mark.parametrize("metric", METRICS)
def test_round_trip(VO, metric, n, dim):
    _round_trip(VO[0], metric, n, dim)


@pytest.mark.parametrize("m,m0", ((4, 8), (48, 64)))
@pytest.mark.parametrize("metric", METRICS)
def test_round_trip_short_and_long_lists(VO, metric, m, m0):
    _round_trip(VO[0], metric, 600, 7, m=m, m0=m0)


def test_a_tombstoned_node_may_carry_a_live_nodes_id(VO):
    V, _ = VO
    rng = np.random.default_rng(1)
    X = rng.standard_normal((40, 4))
    A = V.HNSWIndex(4, 1)
    A.add_rows(_ids(40), X)
    A.delete(int(_ids(40)[3]))
    g = A.graph(with_rows=True)
    g["node_ids"] = g["node_ids"].copy()
    g["node_ids"][3] = g["node_ids"][20]  # the tombstone at node 3 carries the id of live node 20
    B = V.HNSWIndex.from_graph(g, 4, 1, **A.params())
    assert B.len() == 39 and B.graph()["node_ids"][3] == g["node_ids"][20]
    assert np.asarray(B.get_vector(int(g["node_ids"][20])).values).tobytes() == X[20].tobytes()


# ---- 2. a graph no GPU build made ------------------------------------------------------------------------------------
def _keys(metric, Q, X):
    """[nq, n] walk keys: Metric::distance's f64 value before `as u64`, accumulated in index order with a separate
    multiply and add, negative values and NaN at 0 (tests/test_gpu_hnsw_graph_audit.py, restated)."""
    nq, n, dim = Q.shape[0], X.shape[0], X.shape[1]
    a, b, c = np.zeros((nq, n)), np.zeros((nq, n)), np.zeros((nq, n))
    for j in range(dim):
        q, x = Q[:, j][:, None], X[:, j][None, :]
        if metric == 1:
            d = q - x
            a = a + d * d
        elif metric == 2:
            a = a + np.abs(q - x)
        else:
            a = a + q * x
            if metric == 0:
                b = b + (q * q) * np.ones((1, n))
                c = c + np.ones((nq, 1)) * (x * x)
    with np.errstate(invalid="ignore", divide="ignore"):
        if metric == 1:
            s = np.sqrt(a) * 1000.0
        elif metric == 2:
            s = a * 1000.0
        elif metric == 3:
            s = 1000.0 - np.clip(a, -1000.0, 1000.0)
        else:
            na, nb = np.sqrt(b), np.sqrt(c)
            s = np.where((na == 0.0) | (nb == 0.0), 1000.0, (1.0 - a / (na * nb)) * 1000.0)
    return np.where(s > 0.0, s, 0.0)


def _flood(adj, start, n):
    seen = np.zeros(n, bool)
    seen[start] = True
    stack = [start]
    while stack:
        v = stack.pop()
        for e in adj[v]:
            if not seen[e]:
                seen[e] = True
                stack.append(e)
    return seen


EMPTY = 50  # the node with an empty layer-0 list


def _foreign_graph(V, metric, n=400, dim=8, m=16, m0=32, seed=9):
    rng = np.random.default_rng(4000 + metric)
    X = rng.standard_normal((n, dim))
    level = np.array([V.hnsw_level(seed, i, m) for i in range(n)], np.uint8)
    assert level.max() >= 1
    unnamed = int(next(v for v in range(77, n) if level[v] == 0))  # on layer 0 only, so not the entry point either
    D = _keys(metric, X, X)
    np.fill_diagonal(D, np.inf)
    D[:, unnamed] = np.inf  # nobody names this node
    near = np.argsort(D, axis=1, kind="stable")
    upper_off = (np.cumsum(level, dtype=np.uint64) - level).astype(np.uint32)
    cnt0 = (1 + (np.arange(n) * 7) % m0).astype(np.uint32)  # every length 1 .. m0
    cnt0[EMPTY] = 0
    nbr0 = np.zeros((n, m0), np.uint32)
    for i in range(n):
        nbr0[i, :cnt0[i]] = near[i, :cnt0[i]]
    ns = int(level.sum())
    cntU, nbrU = np.zeros(ns, np.uint32), np.zeros((ns, m), np.uint32)
    for i in np.nonzero(level)[0]:
        for layer in range(1, int(level[i]) + 1):
            cand = [int(v) for v in near[i] if level[v] >= layer and v != i][:m]
            s = int(upper_off[i]) + layer - 1
            cntU[s] = len(cand)
            nbrU[s, :len(cand)] = cand
    g = {"m": m, "m0": m0, "n": n, "level": level, "upper_off": upper_off, "cnt0": cnt0, "nbr0": nbr0, "cntU": cntU,
         "nbrU": nbrU, "node_ids": _ids(n), "live": np.ones(n, np.uint8), "rows": X}
    return g, X, unnamed


@pytest.mark.parametrize("metric", METRICS)
def test_a_graph_no_gpu_build_made(VO, metric):
    V, O = VO
    g, X, unnamed = _foreign_graph(V, metric)
    n, dim, m0 = g["n"], X.shape[1], g["m0"]
    assert set(g["cnt0"].tolist()) == set(range(0, m0 + 1))
    B = V.HNSWIndex(dim, metric, m=g["m"], m0=m0, seed=9)
    orphans = B._import_graph(g)
    indeg = np.bincount(np.concatenate([g["nbr0"][i, :g["cnt0"][i]] for i in range(n)]), minlength=n)
    print(f"metric {metric}: {orphans} orphans of {n} nodes")
    assert orphans == int((indeg == 0).sum()) and orphans >= 1 and indeg[unnamed] == 0
    gb = B.graph(with_rows=True)
    _same_graph({**g, "entry": gb["entry"], "max_level": gb["max_level"]}, gb)
    assert gb["max_level"] == int(g["level"].max()) and gb["entry"] == int(np.argmax(g["level"]))

    Q = np.random.default_rng(4100 + metric).standard_normal((NQ, dim))
    adj = [g["nbr0"][i, :g["cnt0"][i]].tolist() for i in range(n)]
    keys = _keys(metric, Q, X)
    u64 = np.array([[O.hnsw_distance(metric, Q[i], X[j]) for j in range(n)] for i in range(NQ)], dtype=np.uint64)
    assert (np.floor(keys).astype(np.uint64) == u64).all()

    # reference navigation: the CPU walker on the same graph, node for node, score for score, evaluation for evaluation
    walker = O.HnswCpuWalker(gb, metric)
    B.set_navigation("reference")
    sizes = set()
    for ef in (1, 10, 128, 512):
        e0, w0 = B.walk_stats()[1], walker.evals.value
        ids, scores, cnt = B.search_batch(Q, ef, metric, ef=ef)
        e1 = B.walk_stats()[1]
        for i in range(NQ):
            nodes, dist = walker.search(Q[i], ef, ef)
            c = int(cnt[i])
            assert ((ids[i, :c] - np.uint64(3)) // np.uint64(7)).tolist() == nodes.tolist(), (ef, i)
            assert scores[i, :c].tolist() == [V.hnsw_score(int(d), metric) for d in dist], (ef, i)
            # a full beam, or everything the landing point reaches: a set closed under the layer-0 lists
            members = set(nodes.tolist())
            assert len(nodes) == ef or (1 <= len(nodes) < ef and all(e in members for v in members for e in adj[v])), (ef, i)
            sizes.add(len(nodes))
        assert e1 - e0 == walker.evals.value - w0, ef
    assert max(sizes) > 128  # some walk did fill a wide beam

    # f32 navigation at ef = 512 >= n: the reachable set of where the descent landed, in (exact key, node) order
    B.set_navigation("f32")
    ids, scores, cnt = B.search_batch(Q, n, metric, ef=512)
    for i in range(NQ):
        c = int(cnt[i])
        nodes = ((ids[i, :c] - np.uint64(3)) // np.uint64(7)).astype(np.int64)
        assert c >= 1 and unnamed not in nodes.tolist()
        want = np.zeros(n, bool)
        want[nodes] = True
        assert any((_flood(adj, int(v), n) == want).all() for v in nodes), i  # the whole reachable set of one of its nodes
        expected = np.sort(nodes)
        assert nodes.tolist() == expected[np.lexsort((expected, keys[i, expected]))].tolist(), i
        assert scores[i, :c].tolist() == [O.hnsw_score(int(u64[i, v]), metric) for v in nodes], i


# ---- 3. refusals -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def source(VO):
    V, _ = VO
    rng = np.random.default_rng(77)
    X = rng.standard_normal((200, 6))
    A = V.HNSWIndex(6, 1, seed=3)
    A.add_rows(_ids(200), X)
    g = A.graph(with_rows=True)
    assert g["cntU"].size >= 2 and g["cnt0"].min() >= 2
    return g, A.params(), X


def _copy(g):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in g.items()}


def _still_usable(V, B, X, expect_len=0):
    assert B.len() == expect_len and B.graph()["n"] == expect_len
    B.add_rows(np.arange(len(X), dtype=np.uint64) + np.uint64(5000), X)
    assert B.len() == expect_len + len(X)
    ids, _, cnt = B.search_batch(X[:3], 5, 1, ef=32)
    assert (cnt == 5).all() and all(5000 + i in ids[i, :2].tolist() for i in range(3))  # (a copy of the row may tie with it)


def _break(g, case):
    n, m0 = g["n"], g["m0"]
    if case == "neighbour >= n":
        g["nbr0"][5, 0] = n
        return "G3: neighbour 200 >= n (node 5, layer 0, slot 0)"
    if case == "self-loop":
        g["nbr0"][5, 1] = 5
        return "G3: a node lists itself (node 5, layer 0, slot 1)"
    if case == "above its level":
        owner = int(np.nonzero(g["level"])[0][0])
        low = int(np.nonzero(g["level"] == 0)[0][0])
        s = int(g["upper_off"][owner])
        g["cntU"][s] = max(int(g["cntU"][s]), 1)
        g["nbrU"][s, 0] = low
        return f"G3: neighbour {low} of level 0 listed above its level (node {owner}, layer 1, slot 0)"
    if case == "cnt0 > m0":
        g["cnt0"][7] = m0 + 1
        return f"G3: count {m0 + 1} > capacity {m0} (node 7, layer 0)"
    if case == "named twice":
        g["nbr0"][9, 1] = g["nbr0"][9, 0]
        return f"G4: neighbour {int(g['nbr0'][9, 0])} named twice (node 9, layer 0, slot 1)"
    if case == "wrong n_upper":
        g["cntU"], g["nbrU"] = g["cntU"][:-1].copy(), g["nbrU"][:-1].copy()
        return "G1: n_upper"
    if case == "duplicate live id":
        g["node_ids"][4] = g["node_ids"][3]
        return f"Vector ID {int(g['node_ids'][3])} already exists"
    if case == "wrong row length":
        g["rows"] = np.ascontiguousarray(g["rows"][:, :-1])
        return "'rows' has shape (200, 5), expected (200, 6)"
    raise AssertionError(case)


@pytest.mark.parametrize("case", ("neighbour >= n", "self-loop", "above its level", "cnt0 > m0", "named twice", "wrong n_upper",
                                  "duplicate live id", "wrong row length"))
def test_refusals_leave_an_empty_usable_handle(VO, source, case):
    V, _ = VO
    g0, p, X = source
    g = _copy(g0)
    text = _break(g, case)
    if case == "wrong n_upper":
        del g["level"], g["upper_off"]  # the library's own check of the total, not Python's of the arrays
    B = V.HNSWIndex(6, 1, **p)
    with pytest.raises(V.IndexOpError) as e:
        B._import_graph(g)
    assert text in str(e.value), str(e.value)
    _still_usable(V, B, X)
    # and the same handle takes the intact graph after a refusal
    B2 = V.HNSWIndex(6, 1, **p)
    with pytest.raises(V.IndexOpError):
        B2._import_graph(g)
    B2._import_graph(g0)
    _same_graph(g0, B2.graph(with_rows=True))


def test_a_wrong_seed_is_caught_by_the_level_check(VO, source):
    V, _ = VO
    g0, p, X = source
    with pytest.raises(V.IndexOpError, match="level law of seed 4"):
        V.HNSWIndex.from_graph(g0, 6, 1, **{**p, "seed": 4})
    B = V.HNSWIndex(6, 1, **{**p, "seed": 4})
    with pytest.raises(V.IndexOpError, match="level law"):
        B._import_graph(g0)
    _still_usable(V, B, X)
    with pytest.raises(V.IndexOpError, match="m = 8"):
        V.HNSWIndex.from_graph(g0, 6, 1, **{**p, "m": 8})


def test_a_non_empty_handle_and_a_flat_handle_are_refused(VO, source):
    import ctypes as C
    V, _ = VO
    g0, p, X = source
    B = V.HNSWIndex(6, 1, **p)
    B.add_rows(np.array([1, 2, 3], np.uint64), X[:3])
    with pytest.raises(V.IndexOpError, match="needs an empty index"):
        B._import_graph(g0)
    _still_usable(V, B, X, expect_len=3)
    F = V.FlatIndex(6)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = F._L.vl_index_hnsw_graph_import(F._h, 200, vp(g0["node_ids"]), vp(g0["live"]), vp(g0["rows"]), 0, vp(g0["cnt0"]),
                                         vp(g0["nbr0"]), g0["cntU"].size, vp(g0["cntU"]), vp(g0["nbrU"]), None)
    assert rc == V.VL_ERR_INVALID_ARG and "needs an HNSW index handle" in V._last_error()
    assert F.len() == 0
    F.add_rows(_ids(200), X)
    assert F.search_arrays(X[0], 1, 1)[0].tolist() == [3]


# ---- 4. snapshots ----------------------------------------------------------------------------------------------------
def test_snapshot(VO, tmp_path):
    V, _ = VO
    from vectorlite_amd.persistence import PersistenceError
    n, dim, metric = 2000, 32, 0
    rng = np.random.default_rng(55)
    X, Q, ids = rng.standard_normal((n, dim)), rng.standard_normal((NQ, dim)), _ids(n)
    A = V.HNSWIndex(dim, metric, ef_construction=64, seed=12)
    A.add_rows(ids, X)
    for v in (0, 17, 1024, n - 1):
        A.delete(int(ids[v]))
    A._meta = {int(ids[1]): ("one", {"k": [1, 2]}), int(ids[2]): (None, None)}
    path = str(tmp_path / "index.npz")
    A.save_snapshot(path)
    assert os.listdir(tmp_path) == ["index.npz"]
    B = V.HNSWIndex.load_snapshot(path)
    assert B._meta == A._meta and B.params() == A.params() and B.metric() == A.metric() and B.len() == n - 4
    _same_graph(A.graph(with_rows=True), B.graph(with_rows=True))
    assert _answers(A, Q, metric, n)[0] == _answers(B, Q, metric, n)[0]

    raw = open(path, "rb").read()
    cut = str(tmp_path / "cut.npz")
    open(cut, "wb").write(raw[:len(raw) // 2])
    with pytest.raises(PersistenceError):
        V.HNSWIndex.load_snapshot(cut)
    with pytest.raises(PersistenceError):
        V.HNSWIndex.load_snapshot(str(tmp_path / "absent.npz"))
    members = dict(np.load(path, allow_pickle=False))
    short = str(tmp_path / "short.npz")
    np.savez(short, **{k: v for k, v in members.items() if k != "cntU"})
    with pytest.raises(PersistenceError, match="cntU"):
        V.HNSWIndex.load_snapshot(short)
    bad = str(tmp_path / "bad.npz")
    members["nbr0"] = members["nbr0"].copy()
    members["nbr0"][10, 0] = 10
    np.savez(bad, **members)
    with pytest.raises(PersistenceError, match="G3: a node lists itself"):
        V.HNSWIndex.load_snapshot(bad)
    members["nbr0"] = members["nbr0"].astype(np.int64)
    np.savez(bad, **members)
    with pytest.raises(PersistenceError, match="nbr0"):
        V.HNSWIndex.load_snapshot(bad)
