"""Reference navigation of the GPU graph walk (vl_index_hnsw_set_navigation(h, VL_HNSW_NAV_REFERENCE)) against the
CPU walker (oracle/vl_hnsw_cpu.c) on the SAME exported graph: node for node, distance for distance, evaluation for
evaluation.  Ids are arange in insertion order, so a node index is its id."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METRICS = (0, 1, 2, 3)  # cosine, euclidean, manhattan, dot (the ABI's codes = the oracle's)


def _build(rows, metric):
    import vectorlite_amd as V
    idx = V.HNSWIndex(rows.shape[1], metric)
    idx.add_rows(np.arange(rows.shape[0], dtype=np.uint64), rows)
    return idx


def _walker(idx, metric):
    from oracle import oracle as O
    O.build()
    return O.HnswCpuWalker(idx.graph(with_rows=True), metric)


def _evals(idx):
    return idx.walk_stats()[1]


def _check_beams(idx, walker, Q, metric, ef):
    """search_batch(Q, k = ef, ef = ef) in reference mode returns the walker's whole beam, in order; evaluations agree.
    Returns the walker's beams."""
    import vectorlite_amd as V
    e0, w0 = _evals(idx), walker.evals.value
    ids, scores, n = idx.search_batch(Q, ef, metric, ef=ef)
    e1, w1 = _evals(idx), walker.evals.value
    beams = [walker.search(Q[i], ef, ef) for i in range(len(Q))]
    e2 = walker.evals.value
    for i, (nodes, dist) in enumerate(beams):
        m = int(n[i])
        assert len(nodes) == min(ef, walker.g["n"]), (metric, ef, i)   # full beams: nothing passes vacuously
        assert ids[i, :m].tolist() == nodes.tolist(), (metric, ef, i)
        assert scores[i, :m].tolist() == [V.hnsw_score(int(d), metric) for d in dist], (metric, ef, i)
    assert w1 == w0
    assert e1 - e0 == e2 - w1, (metric, ef)
    return beams


def _rows(rng, n, dim, metric):
    x = rng.standard_normal((n, dim))
    if metric in (0, 3):
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


@pytest.mark.parametrize("metric", METRICS)
def test_node_for_node_parity_with_the_cpu_walker(metric):
    rng = np.random.default_rng(100 + metric)
    for dim, n in ((16, 20_000), (50, 8_000), (384, 3_000)):
        X = _rows(rng, n, dim, metric)
        idx = _build(X, metric)
        idx.set_navigation("reference")
        walker = _walker(idx, metric)
        Q = _rows(rng, 12, dim, metric)
        for ef in (1, 10, 32, 128, 512):
            _check_beams(idx, walker, Q, metric, ef)


@pytest.mark.parametrize("metric,kind", [(2, "grid"), (1, "grid"), (0, "dup")])
def test_tied_u64_distances_keep_the_walkers_first_seen_order(metric, kind):
    rng = np.random.default_rng(7 + metric)
    dim, n = 8, 6_000
    if kind == "grid":   # small integer grid: many rows at the same integer (Manhattan) / sqrt-of-integer distance
        X = rng.integers(0, 3, size=(n, dim)).astype(np.float64)
        Q = rng.integers(0, 3, size=(16, dim)).astype(np.float64)
    else:                # every row four times
        base = rng.standard_normal((n // 4, dim))
        X = np.repeat(base, 4, axis=0)
        rng.shuffle(X)
        Q = rng.standard_normal((16, dim))
    idx = _build(X, metric)
    idx.set_navigation("reference")
    walker = _walker(idx, metric)
    ties = 0
    for ef in (10, 32, 128):
        beams = _check_beams(idx, walker, Q, metric, ef)
        ties += sum(int(np.sum(d[1:] == d[:-1])) for _, d in beams)
    assert ties > 50, ties  # the order inside tied runs decided what came back


def _post_process(nodes, live, k_eff, refill):
    """src/index/hnsw.rs:468-495 on a beam: the closest min(k, len) (refill: the whole beam), tombstones dropped."""
    take = nodes if refill else nodes[:k_eff]
    return [int(x) for x in take if live[int(x)]][:k_eff]


def test_wrapper_semantics_with_tombstones_in_reference_mode():
    metric, dim, n, k = 0, 32, 10_000, 10
    rng = np.random.default_rng(55)
    X = _rows(rng, n, dim, metric)
    idx = _build(X, metric)
    dead = rng.choice(n, n // 10, replace=False)
    for d in dead:
        idx.delete(int(d))
    idx.set_navigation("reference")
    walker = _walker(idx, metric)
    live = walker.g["live"]
    assert int(live.sum()) == n - len(dead)
    Q = _rows(rng, 16, dim, metric)
    for i in range(len(Q)):
        nodes, _ = walker.search(Q[i], k, k)                         # default search(): ef = min(k, len)
        got = [r.id for r in idx.search(Q[i], k, metric)]
        assert got == _post_process(nodes, live, k, False), i
        for ef in (32, 128):                                         # search_ef: the freed slots are refilled
            nodes, _ = walker.search(Q[i], ef, ef)
            gi, _ = idx.search_arrays(Q[i], k, metric, ef=ef)
            assert gi.tolist() == _post_process(nodes, live, k, True), (i, ef)


def test_dim_3072_walks_at_ef_256_and_512():
    metric, dim, n = 1, 3072, 1_500
    rng = np.random.default_rng(3072)
    X = rng.standard_normal((n, dim))
    idx = _build(X, metric)
    idx.set_navigation("reference")
    walker = _walker(idx, metric)
    Q = rng.standard_normal((3, dim))
    for ef in (256, 512):
        beams = _check_beams(idx, walker, Q, metric, ef)
        assert all(len(b[0]) == ef for b in beams)


def test_concurrent_searches_in_reference_mode_get_their_lone_answers():
    metric, dim, n, k, T = 1, 64, 20_000, 10, 16
    rng = np.random.default_rng(16)
    idx = _build(rng.standard_normal((n, dim)), metric)
    idx.set_navigation("reference")
    Q = rng.standard_normal((T * 8, dim))
    lone = [[(r.id, r.score) for r in idx.search(Q[i], k, metric)] for i in range(len(Q))]
    got = [None] * len(Q)
    start = threading.Barrier(T)

    def worker(t):
        start.wait()
        for i in range(t, len(Q), T):
            got[i] = [(r.id, r.score) for r in idx.search(Q[i], k, metric)]

    th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got == lone


def test_default_navigation_is_unchanged_and_clones_start_in_it():
    import vectorlite_amd as V
    metric, dim, n, k = 0, 48, 12_000, 10
    rng = np.random.default_rng(48)
    idx = _build(_rows(rng, n, dim, metric), metric)
    Q = _rows(rng, 32, dim, metric)

    def run(h, ef):
        e0 = _evals(h)
        out = h.search_batch(Q, k, metric, ef=ef)
        return [a.tolist() for a in out], _evals(h) - e0

    before = {ef: run(idx, ef) for ef in (0, 64)}
    idx.set_navigation("reference")
    ref = {ef: run(idx, ef) for ef in (0, 64)}
    c = idx.clone()                       # starts in f32 navigation
    idx.set_navigation("f32")
    after = {ef: run(idx, ef) for ef in (0, 64)}
    assert after == before
    assert {ef: run(c, ef) for ef in (0, 64)} == before
    # f32 mode re-scores its final beam (extra evaluations), reference mode does not: the counts tell the modes apart
    assert all(ref[ef][1] != before[ef][1] for ef in (0, 64))
    with pytest.raises(ValueError):
        idx.set_navigation("f64")
    L = idx._L
    assert L.vl_index_hnsw_set_navigation(idx._h, 2) != 0             # unknown mode: VL_ERR_INVALID_ARG
    flat = V.FlatIndex(dim)
    assert L.vl_index_hnsw_set_navigation(flat._h, 1) != 0             # not an HNSW handle
    assert "HNSW" in V._last_error()


def test_config4_sized_cell_200k_x_384_latent16_cosine():
    import torch
    metric, n, dim, latent = 0, 200_000, 384, 16
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(200)
    A = torch.randn((latent, dim), dtype=torch.float64, device=dev, generator=g)
    x = torch.randn((n, latent), dtype=torch.float64, device=dev, generator=g) @ A
    x += 0.05 * torch.randn((n, dim), dtype=torch.float64, device=dev, generator=g)
    x /= torch.linalg.vector_norm(x, dim=1, keepdim=True)
    import vectorlite_amd as V
    idx = V.HNSWIndex(dim, metric)
    idx.add_rows(np.arange(n, dtype=np.uint64), x)
    idx.set_navigation("reference")
    walker = _walker(idx, metric)
    rng = np.random.default_rng(201)
    Q = rng.standard_normal((32, latent)) @ A.cpu().numpy() + 0.05 * rng.standard_normal((32, dim))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    for ef in (10, 128):
        _check_beams(idx, walker, Q, metric, ef)
