"""Id-filtered graph walks on HNSW indexes (vl_index_search_ef_filtered).

Reference navigation is held against the CPU restatement of the walk's definition (tests/_hnsw_filtered_walk.py) on the
SAME exported graph: node for node, score bit for score bit, evaluation for evaluation, and the list capacity the host
plan chose.  Ids are arange in insertion order, so a node index is its id.  f32 navigation is judged by what it must
return (passing, live, exactly scored, ordered) and by recall beside the restatement's."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _hnsw_filtered_walk import filtered_walk  # noqa: E402

pytestmark = pytest.mark.gpu

COS, EUC, MAN, DOT = 0, 1, 2, 3
_INDEXES = {}


def _rows(rng, n, dim, metric):
    x = rng.standard_normal((n, dim))
    if metric in (COS, DOT):
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def _build(rows, metric, m=16, m0=32):
    import vectorlite_amd as V
    idx = V.HNSWIndex(rows.shape[1], metric, m=m, m0=m0, ef_construction=64)
    idx.add_rows(np.arange(rows.shape[0], dtype=np.uint64), rows)
    return idx


def _index(metric, dim, n, m=16, m0=32):
    """One index (and its exported graph) per shape for the whole module; tests that mutate build their own."""
    key = (metric, dim, n, m, m0)
    if key not in _INDEXES:
        rng = np.random.default_rng(hash(key) % (1 << 32))
        idx = _build(_rows(rng, n, dim, metric), metric, m, m0)
        _INDEXES[key] = (idx, idx.graph(with_rows=True))
    return _INDEXES[key]


def _plan(k, ef, n, n_pass, min_beam=0):
    """vectorlite_amd/csrc/hnsw_filter_plan.hpp, restated: (route, cap, max_candidates, ef_walk)."""
    mc = min(k, n_pass)
    ew = max(mc, ef if ef else min_beam)
    if n_pass == 0 or ew == 0 or ew > 512 or ew * n > 256 * n_pass:
        return 1, 0, mc, ew
    need = max(ew, -(-2 * ew * n // n_pass))
    return 0, next(c for c in (64, 128, 256, 512) if need <= c or c == 512), mc, ew


def _evals(idx):
    return idx.walk_stats()[1]


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64).tolist()


def _check_reference(idx, g, metric, Q, ef, pass_ids, k=None, want_cap=None):
    """A filtered batch in reference navigation against the restatement.  Returns the restatement's walks."""
    import vectorlite_amd as V
    k = ef if k is None else k
    passing = np.isin(g["node_ids"], np.asarray(pass_ids, np.uint64)) & (g["live"] != 0)
    n_pass = int(passing.sum())
    route, cap, mc, ew = _plan(k, ef, g["n"], n_pass)
    assert route == 0, ("the case was meant to walk", ef, g["n"], n_pass)
    if want_cap is not None:
        assert cap == want_cap, (cap, want_cap)
    idx.set_navigation("reference")
    try:
        with idx.make_walk_filter(pass_ids) as wf:
            assert wf.nodes() == n_pass
            e0 = _evals(idx)
            ids, scores, n = idx.search_batch(Q, k, metric, ef=ef, filter=wf)
            e1 = _evals(idx)
            last = idx.last_filtered()
    finally:
        idx.set_navigation("f32")
    walks = [filtered_walk(g, metric, q, ew, cap, passing, k=mc) for q in Q]
    for i, w in enumerate(walks):
        m = int(n[i])
        assert ids[i, :m].tolist() == g["node_ids"][w["nodes"]].tolist(), (metric, ef, cap, i)
        assert _bits(scores[i, :m]) == _bits([V.hnsw_score(int(d), metric) for d in w["dist"]]), (metric, ef, i)
        assert w["longest"] <= cap
    assert e1 - e0 == sum(w["evals"] for w in walks), (metric, ef, cap)
    assert last["route"] == 0 and last["cap"] == cap and last["pass_nodes"] == n_pass
    assert last["cap_cut_walks"] == sum(w["cut"] for w in walks), (metric, ef, cap, [w["cut"] for w in walks])
    return walks


def _subset(rng, n, count):
    return np.sort(rng.choice(n, count, replace=False)).astype(np.uint64)


# (ef, passing fraction, the capacity the plan must choose): all four capacities, the window at both ends of each
CELLS_16 = [(1, 1.0, 64), (1, 0.1, 64), (10, 0.5, 64), (10, 0.25, 128), (10, 0.1, 256), (32, 1.0, 64), (32, 0.5, 128),
            (32, 0.25, 256), (64, 0.5, 256), (64, 0.25, 512), (200, 1.0, 512)]
CELLS_384 = [(1, 0.5, 64), (10, 0.25, 128), (32, 0.25, 256), (64, 0.25, 512), (200, 1.0, 512)]


@pytest.mark.parametrize("metric", (COS, EUC, MAN, DOT))
@pytest.mark.parametrize("dim,n,cells", [(16, 4000, CELLS_16), (384, 3000, CELLS_384)])
def test_reference_navigation_matches_the_restatement(metric, dim, n, cells):
    idx, g = _index(metric, dim, n)
    rng = np.random.default_rng(31 * metric + dim)
    Q = _rows(rng, 2, dim, metric)
    for ef, frac, cap in cells:
        _check_reference(idx, g, metric, Q, ef, _subset(rng, n, int(round(frac * n))), want_cap=cap)


def test_a_half_space_filter_widens_the_window_and_the_capacity_cuts_it():
    """The passing rows are the quarter of the rows farthest from the query along one axis: the walk starts among rows
    that do not pass, expands them, and fills its list with them.  At ef 64 the plan gives the list 512 entries; the
    cap drops entries the window would have kept -- the ef-th passing one among them."""
    metric, dim, n = EUC, 16, 8000
    idx, g = _index(metric, dim, n)
    X = g["rows"]
    order = np.argsort(X[:, 0], kind="stable")
    Q = np.zeros((4, dim))
    Q[:, 0] = (0.1, 0.25, 0.4, 3.0)   # just inside the other three quarters ... and far inside them
    Q[:, 1] = (0.0, 0.5, -0.5, 0.0)
    half = _check_reference(idx, g, metric, Q, 10, order[: n // 2].astype(np.uint64), want_cap=64)
    assert all(w["longest"] > 10 for w in half)           # entries that do not pass sit inside the window
    quarter = _check_reference(idx, g, metric, Q, 64, order[: n // 4].astype(np.uint64), want_cap=512)
    assert all(w["cut"] and w["longest"] == 512 for w in quarter)
    assert any(w["lost_efth"] for w in quarter[:3])       # the cap took an ef-th passing entry off the list
    assert len(quarter[3]["nodes"]) < 64                  # ... or the list never reached the passing quarter's 64 nearest


@pytest.mark.parametrize("metric,kind", [(MAN, "grid"), (EUC, "grid"), (COS, "dup")])
def test_tied_distances_keep_first_seen_order_under_a_filter(metric, kind):
    rng = np.random.default_rng(70 + metric)
    dim, n = 8, 4000
    if kind == "grid":
        X = rng.integers(0, 3, size=(n, dim)).astype(np.float64)
        Q = rng.integers(0, 3, size=(3, dim)).astype(np.float64)
    else:
        X = np.repeat(rng.standard_normal((n // 4, dim)), 4, axis=0)
        rng.shuffle(X)
        Q = rng.standard_normal((3, dim))
    idx = _build(X, metric)
    g = idx.graph(with_rows=True)
    ties = 0
    for ef, frac in ((10, 0.5), (32, 0.5), (32, 1.0)):
        walks = _check_reference(idx, g, metric, Q, ef, _subset(rng, n, int(frac * n)))
        ties += sum(int(np.sum(np.diff(w["dist"]) == 0)) for w in walks)
    assert ties > 20, ties  # the order inside tied runs decided what came back


@pytest.mark.parametrize("m,m0", [(4, 8), (48, 64)])
def test_short_and_long_neighbour_lists(m, m0):
    metric, dim, n = EUC, 16, 3000
    idx, g = _index(metric, dim, n, m, m0)
    rng = np.random.default_rng(m0)
    Q = _rows(rng, 2, dim, metric)
    for ef, frac in ((10, 1.0), (10, 0.25), (32, 0.5)):
        _check_reference(idx, g, metric, Q, ef, _subset(rng, n, int(frac * n)))


def test_entry_node_outside_the_filter_tombstoned_and_bitmap_word_edges():
    """n is no multiple of 32; nodes 31 / 32 / n - 1 sit on opposite sides of the filter; the entry node first does
    not pass, then is a tombstone."""
    metric, dim, n = COS, 16, 3001
    rng = np.random.default_rng(3001)
    X = _rows(rng, n, dim, metric)
    idx = _build(X, metric)
    g = idx.graph(with_rows=True)
    entry = g["entry"]
    evens = np.arange(0, n, 2, dtype=np.uint64)           # 32 and n - 1 = 3000 pass, 31 does not
    odds = np.arange(1, n, 2, dtype=np.uint64)            # 31 passes, 32 and 3000 do not
    Q = np.stack([X[31], X[32], X[n - 1], X[entry]])
    for ids in (evens, odds):
        walks = _check_reference(idx, g, metric, Q, 10, ids)
        for node, w in zip((31, 32, n - 1), walks):       # the query is the node's own row
            assert node in ids or node not in w["nodes"]
        assert any(node in w["nodes"] for node, w in zip((31, 32, n - 1), walks))
    everyone_else = np.setdiff1d(np.arange(n, dtype=np.uint64), np.array([entry], np.uint64))
    walks = _check_reference(idx, g, metric, Q, 10, everyone_else)
    assert all(entry not in w["nodes"] for w in walks)
    idx.delete(int(entry))
    g = idx.graph(with_rows=True)
    assert g["entry"] == entry and not g["live"][entry]
    walks = _check_reference(idx, g, metric, Q, 10, np.arange(n, dtype=np.uint64))
    assert all(entry not in w["nodes"] for w in walks)


def test_fewer_passing_nodes_than_ef_returns_the_reachable_ones():
    metric, dim, n = EUC, 16, 200
    idx, g = _index(metric, dim, n)
    rng = np.random.default_rng(200)
    ids = _subset(rng, n, 8)                               # 10 * 200 <= 256 * 8: still a walk, with 512 entries
    walks = _check_reference(idx, g, metric, _rows(rng, 3, dim, metric), 10, ids, want_cap=512)
    assert all(0 < len(w["nodes"]) <= 8 for w in walks)
    assert any(len(w["nodes"]) == 8 for w in walks)


@pytest.mark.parametrize("nav", ("f32", "reference"))
def test_an_all_pass_filter_is_the_unfiltered_search(nav):
    metric, dim, n, k = COS, 48, 6000, 10
    idx, g = _index(metric, dim, n)
    rng = np.random.default_rng(48)
    Q = _rows(rng, 24, dim, metric)
    idx.set_navigation(nav)
    try:
        with idx.make_walk_filter(range(n)) as wf:
            for ef in (0, 10, 64, 128, 256):
                e0 = _evals(idx)
                plain = idx.search_batch(Q, k, metric, ef=ef)
                e1 = _evals(idx)
                filt = idx.search_batch(Q, k, metric, ef=ef, filter=wf)
                e2 = _evals(idx)
                assert idx.last_filtered()["route"] == 0
                assert filt[0].tolist() == plain[0].tolist() and filt[2].tolist() == plain[2].tolist(), (nav, ef)
                assert _bits(filt[1]) == _bits(plain[1]), (nav, ef)
                assert e2 - e1 == e1 - e0, (nav, ef)
    finally:
        idx.set_navigation("f32")


def test_f32_navigation_returns_exactly_scored_ordered_passing_rows_and_keeps_the_recall():
    """Recall@10 against the exact subset order, 64 queries, ef 10, beside the restatement's on the same graph.  The f32
    key orders more finely than the u64, so f32 navigation is not expected to be worse; the margin allowed is one
    differing node per ten queries (0.01)."""
    import vectorlite_amd as V
    from oracle import oracle as O
    O.build()
    metric, dim, n, k, ef = COS, 16, 4000, 10, 10
    idx, g = _index(metric, dim, n)
    X = g["rows"]
    rng = np.random.default_rng(64)
    Q = _rows(rng, 64, dim, metric)
    for frac in (0.5, 0.1):
        ids = _subset(rng, n, int(frac * n))
        passing = np.isin(g["node_ids"], ids)
        route, cap, mc, ew = _plan(k, ef, n, len(ids))
        assert route == 0
        got_ids, got_scores, got_n = idx.search_batch(Q, k, metric, ef=ef, filter=ids)
        hit_f32 = hit_ref = 0
        for i, q in enumerate(Q):
            m = int(got_n[i])
            mine = got_ids[i, :m].tolist()
            assert m == k and all(passing[v] for v in mine) and len(set(mine)) == m
            dist = [O.hnsw_distance(metric, q, X[v]) for v in mine]
            assert _bits(got_scores[i, :m]) == _bits([V.hnsw_score(d, metric) for d in dist])
            assert dist == sorted(dist)  # ranked by the f64 value the u64 truncates (then node): never out of u64 order
            d_all = 1.0 - (X[ids.astype(np.int64)] @ q)
            truth = set(ids[np.lexsort((ids, d_all))[:k]].tolist())
            hit_f32 += len(truth & set(mine))
            hit_ref += len(truth & set(filtered_walk(g, metric, q, ew, cap, passing, k=mc)["nodes"]))
        r_f32, r_ref = hit_f32 / (k * len(Q)), hit_ref / (k * len(Q))
        print(f"pass fraction {frac}: recall@10 f32 navigation {r_f32:.4f}, restatement {r_ref:.4f}")
        assert r_f32 >= r_ref - 0.01, (frac, r_f32, r_ref)


def _exact_recipe(g, metric, q, ids, k):
    """The exact route restated: FlatIndex::search over the subset's rows in storage order (tombstoned ones included),
    asked for k plus the subset's tombstones; u64 distances of the winners; tombstones dropped; scores; stable sort."""
    from oracle import oracle as O
    import vectorlite_amd as V
    member = np.isin(g["node_ids"], ids)
    pos = np.flatnonzero(member)
    live = g["live"][pos] != 0
    n_pass, tombs = int(live.sum()), int((~live).sum())
    flat = O.FlatOracle(g["rows"].shape[1], pos.astype(np.uint64), g["rows"][pos])
    winners, _ = flat.search(q, min(len(pos), k + tombs), metric)
    res = []
    for p in winners.tolist():
        if len(res) == min(k, n_pass):
            break
        if g["live"][p]:
            res.append((int(g["node_ids"][p]), V.hnsw_score(O.hnsw_distance(metric, q, g["rows"][p]), metric)))
    res.sort(key=lambda t: -t[1])  # stable
    return [r[0] for r in res], [r[1] for r in res]


@pytest.mark.parametrize("metric", (COS, EUC))
def test_the_exact_route_is_the_flat_search_over_the_subset(metric):
    from oracle import oracle as O
    O.build()
    dim, n = 16, 5000
    rng = np.random.default_rng(5000 + metric)
    idx = _build(_rows(rng, n, dim, metric), metric)
    few, many = _subset(rng, n, 40), _subset(rng, n, 700)
    for d in sorted({int(few[3]), int(few[17]), int(many[5]), int(many[600])}):  # tombstones inside both subsets
        idx.delete(d)
    g = idx.graph(with_rows=True)
    Q = _rows(rng, 3, dim, metric)
    e0 = _evals(idx)
    for ids, k, ef in ((few, 10, 10), (few, 60, 0), (many, 600, 0), (many, 5000, 32)):
        out_ids, out_scores, out_n = idx.search_batch(Q, k, metric, ef=ef, filter=ids)
        last = idx.last_filtered()
        n_pass = int((np.isin(g["node_ids"], ids) & (g["live"] != 0)).sum())
        assert last["route"] == 1 and last["cap"] == 0 and last["pass_nodes"] == n_pass and last["cap_cut_walks"] == 0
        for i, q in enumerate(Q):
            want_ids, want_scores = _exact_recipe(g, metric, q, ids, k)
            m = int(out_n[i])
            assert m == min(k, n_pass) == len(want_ids)
            assert out_ids[i, :m].tolist() == want_ids and _bits(out_scores[i, :m]) == _bits(want_scores), (k, ef, i)
    assert _evals(idx) > e0
    # nothing passes: zero results, exact route
    out_ids, out_scores, out_n = idx.search_batch(Q, 10, metric, ef=10, filter=[n + 5, n + 6])
    assert out_n.tolist() == [0, 0, 0] and idx.last_filtered() == {"route": 1, "cap": 0, "pass_nodes": 0, "cap_cut_walks": 0}


def test_filters_follow_deletes_adds_and_re_added_ids():
    metric, dim, n = EUC, 16, 3000
    rng = np.random.default_rng(77)
    X = _rows(rng, n + 64, dim, metric)
    idx = _build(X[:n], metric)
    ids = np.concatenate([np.arange(0, n, 2), np.arange(n, n + 64)]).astype(np.uint64)  # half the rows + 64 ids not there yet
    with idx.make_walk_filter(ids) as wf:
        assert wf.nodes() == n // 2
        q = X[10]
        first, _ = idx.search_arrays(q, 5, metric, ef=32, filter=wf)
        assert first[0] == 10
        for victim in first[:3].tolist():
            idx.delete(int(victim))
        assert wf.nodes() == n // 2 - 3
        after, _ = idx.search_arrays(q, 5, metric, ef=32, filter=wf)
        assert not set(after.tolist()) & set(first[:3].tolist()) and len(after) == 5
        assert all(v % 2 == 0 for v in after.tolist())
        # rows whose ids were in the set all along arrive
        idx.add_rows(np.arange(n, n + 64, dtype=np.uint64), X[n:])
        assert wf.nodes() == n // 2 - 3 + 64
        new, _ = idx.search_arrays(X[n + 7], 3, metric, ef=32, filter=wf)
        assert new[0] == n + 7
        # a deleted id comes back as a new node
        idx.add_rows(np.array([10], np.uint64), X[10][None, :])
        assert wf.nodes() == n // 2 - 2 + 64
        back, scores = idx.search_arrays(q, 5, metric, ef=32, filter=wf)
        assert back[0] == 10 and back.tolist().count(10) == 1
        g = idx.graph(with_rows=True)
        walks = _check_reference(idx, g, metric, np.stack([q, X[n + 7]]), 10, ids)
        assert walks[0]["nodes"][0] == g["n"] - 1  # node index of the re-added row; its id is 10


def test_unfiltered_batches_are_untouched_by_filtered_ones_between_them():
    """Visited-set hygiene.  One of the filtered batches marks more nodes per walk than a walk's visited log holds
    (8192), so its sets are cleared by wiping the bitmaps: 512-entry lists filled with rows that do not pass, on
    40 000 rows of dim 64 (a walk's evaluations are the nodes it marked, plus the entry point)."""
    metric, dim, n, k = EUC, 64, 40_000, 10
    idx, g = _index(metric, dim, n, 48, 64)   # lists of 64: with lists of 32 a walk marked 7171 nodes, under the log's 8192
    rng = np.random.default_rng(512)
    Q = _rows(rng, 40, dim, metric)

    def plain(nav="f32"):
        idx.set_navigation(nav)
        e0 = _evals(idx)
        out = idx.search_batch(Q, k, metric, ef=64)
        idx.set_navigation("f32")
        return [a.tolist() for a in out], _evals(idx) - e0

    before = {nav: plain(nav) for nav in ("f32", "reference")}
    order = np.argsort(g["rows"][:, 0], kind="stable")
    far = np.zeros((16, dim))
    far[:, 0] = 3.0
    far[:, 1] = np.linspace(-1.0, 1.0, 16)
    for nav in ("reference", "f32"):
        idx.set_navigation(nav)
        with idx.make_walk_filter(order[: n // 4].astype(np.uint64)) as wf:
            e0 = _evals(idx)
            idx.search_batch(far, 64, metric, ef=64, filter=wf)
            per_walk = (_evals(idx) - e0) / len(far)
            last = idx.last_filtered()
            print(f"{nav}: {per_walk:.1f} evaluations per filtered walk, cut walks {last['cap_cut_walks']}")
            assert last["route"] == 0 and last["cap"] == 512
            assert per_walk > 8192 + 64 + 1, per_walk
        idx.set_navigation("f32")
        assert {v: plain(v) for v in ("f32", "reference")} == before
        with idx.make_walk_filter(order[: n // 2].astype(np.uint64)) as wf:
            idx.set_navigation(nav)
            idx.search_batch(Q, k, metric, ef=10, filter=wf)
            idx.set_navigation("f32")
        assert {v: plain(v) for v in ("f32", "reference")} == before


def test_eight_threads_with_different_filters_get_their_lone_answers():
    metric, dim, n, k, T = COS, 32, 6000, 10, 8
    idx, g = _index(metric, dim, n)
    rng = np.random.default_rng(8)
    Q = _rows(rng, T * 6, dim, metric)
    filters = [idx.make_walk_filter(np.arange(t, n, t + 2, dtype=np.uint64)) for t in range(T)]
    lone = [[a.tolist() for a in idx.search_arrays(Q[i], k, metric, ef=32, filter=filters[i % T])] for i in range(len(Q))]
    got = [None] * len(Q)
    start = threading.Barrier(T)

    def worker(t):
        start.wait()
        for i in range(t, len(Q), T):
            got[i] = [a.tolist() for a in idx.search_arrays(Q[i], k, metric, ef=32, filter=filters[t])]

    th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for f in filters:
        f.close()
    assert got == lone
    assert all(len(r[0]) == k and all(v % (i % T + 2) == i % T for v in r[0]) for i, r in enumerate(lone))


def test_errors_and_refusals():
    import vectorlite_amd as V
    metric, dim, n = COS, 16, 300
    rng = np.random.default_rng(9)
    idx = _build(_rows(rng, n, dim, metric), metric)
    other = _build(_rows(rng, n, dim, metric), metric)
    flat = V.FlatIndex(dim)
    flat.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, dim)))
    L = idx._L
    q = np.ascontiguousarray(rng.standard_normal(dim))
    out_i, out_s, out_n = np.zeros(16, np.uint64), np.zeros(16), C.c_uint64(7)

    def call(h, tok, qlen=dim, k=4, ef=0, m=metric):
        return L.vl_index_search_ef_filtered(h, tok, q.ctypes.data_as(C.POINTER(C.c_double)), 1, qlen, k, ef, m, 16,
                                             out_i.ctypes.data_as(C.POINTER(C.c_uint64)),
                                             out_s.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out_n))

    wf = idx.make_walk_filter(range(0, n, 3))
    tok = wf.token
    assert tok != 0 and call(idx._h, tok) == 0 and out_n.value == 4
    assert call(idx._h, 0) == 8 and call(idx._h, tok + 1000) == 8 and "filter" in V._last_error()
    assert call(other._h, tok) == 8                        # a token of another handle
    assert call(flat._h, tok) == 8 and "HNSW" in V._last_error()
    assert call(idx._h, tok, ef=513) == 8 and "512" in V._last_error()
    assert call(idx._h, tok, qlen=dim - 1, m=EUC) == 1     # the dimension is checked before the metric
    assert call(idx._h, tok, m=EUC) == 4
    assert call(idx._h, tok, k=0) == 0 and out_n.value == 0
    nodes = C.c_uint64(0)
    assert L.vl_index_hnsw_filter_nodes(idx._h, tok, C.byref(nodes)) == 0 and nodes.value == 100
    assert L.vl_index_hnsw_filter_nodes(flat._h, tok, C.byref(nodes)) == 8
    assert L.vl_index_hnsw_filter_create(flat._h, None, 0, C.byref(nodes), None) == 8
    assert L.vl_index_hnsw_last_filtered(flat._h, None, None, None, None) == 8
    # flat filter entry points still refuse HNSW handles, and the flat ones do not know walk-filter tokens
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        idx.make_filter([1])
    rows = C.c_uint64(0)
    assert L.vl_index_filter_rows(flat._h, tok, C.byref(rows)) == 8
    ff = flat.make_filter([1, 2])
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        idx.search_arrays(q, 3, metric, filter=ff)
    with pytest.raises(V.IndexOpError):
        other.search_arrays(q, 3, metric, filter=wf)       # a WalkFilter of another index
    # tokens are not reused, a destroyed one is unknown, destroying twice is refused
    wf.close()
    assert call(idx._h, tok) == 8
    assert L.vl_index_hnsw_filter_destroy(idx._h, tok) == 8
    with idx.make_walk_filter([1, 2, 3]) as wf2:
        assert wf2.token not in (0, tok)
        assert [r.id for r in idx.search(q, 5, metric, filter=wf2)] == sorted(
            [1, 2, 3], key=lambda v: -float(idx.get_vector(v).values @ q / np.linalg.norm(q)))
    with pytest.raises(V.IndexOpError, match="closed"):
        wf2.nodes()
    # a clone does not inherit filters
    wf3 = idx.make_walk_filter([5])
    c = idx.clone()
    assert call(c._h, wf3.token) == 8
    wf3.close()
