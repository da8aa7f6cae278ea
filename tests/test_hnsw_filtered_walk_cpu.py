"""The CPU restatement of the id-filtered HNSW walk (tests/_hnsw_filtered_walk.py) on a hand-made graph: no GPU needed.
With an all-pass filter the window is the first ef entries and the walk is oracle/vl_hnsw_cpu.c's, node for node,
distance for distance and evaluation for evaluation -- that anchors the restatement the GPU tests compare against."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _hnsw_filtered_walk import filtered_walk  # noqa: E402

COS = 0
N, DIM, M, M0 = 2000, 16, 8, 16


@pytest.fixture(scope="module")
def graph():
    """2000 x 16 unit rows; level law by hand (every 8th node on layer 1, every 64th on layer 2); each list the node's
    nearest rows on that layer by plain numpy, capped at m0 / m, plus a ring edge so that every layer is connected."""
    rng = np.random.default_rng(2000)
    X = rng.standard_normal((N, DIM))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    level = np.zeros(N, np.uint8)
    level[::8] = 1
    level[::64] = 2
    sim = X @ X.T
    np.fill_diagonal(sim, -2.0)

    def lists(members, width):
        out = {}
        sub = sim[np.ix_(members, members)]
        order = np.argsort(-sub, axis=1)[:, : width - 1]
        for r, i in enumerate(members):
            near = [int(members[c]) for c in order[r] if members[c] != i]
            ring = int(members[(r + 1) % len(members)])
            out[int(i)] = (near if ring in near else near + [ring])[:width] if len(members) > 1 else []
        return out

    l0 = lists(np.arange(N), M0)
    up = {L: lists(np.flatnonzero(level >= L), M) for L in (1, 2)}
    g = {"n": N, "m": M, "m0": M0, "entry": 0, "max_level": 2, "rows": X, "level": level}
    g["cnt0"] = np.array([len(l0[i]) for i in range(N)], np.uint32)
    g["nbr0"] = np.zeros((N, M0), np.uint32)
    for i in range(N):
        g["nbr0"][i, : len(l0[i])] = l0[i]
    offs, rows_u = [], []
    for i in range(N):
        offs.append(len(rows_u))
        for L in range(1, int(level[i]) + 1):
            rows_u.append(up[L][i])
    g["upper_off"] = np.array(offs, np.uint32)
    g["cntU"] = np.array([len(x) for x in rows_u], np.uint32)
    g["nbrU"] = np.zeros((len(rows_u), M), np.uint32)
    for s, x in enumerate(rows_u):
        g["nbrU"][s, : len(x)] = x
    return g


@pytest.fixture(scope="module")
def queries():
    rng = np.random.default_rng(2001)
    Q = rng.standard_normal((8, DIM))
    return Q / np.linalg.norm(Q, axis=1, keepdims=True)


@pytest.mark.parametrize("ef,cap", [(1, 64), (10, 64), (64, 64), (64, 512)])
def test_an_all_pass_filter_is_the_cpu_walkers_walk(graph, queries, ef, cap):
    from oracle import oracle as O
    O.build()
    walker = O.HnswCpuWalker(graph, COS)
    everyone = np.ones(N, bool)
    for q in queries:
        e0 = walker.evals.value
        nodes, dist = walker.search(q, ef, ef)
        got = filtered_walk(graph, COS, q, ef, cap, everyone)
        assert len(nodes) == ef
        assert got["nodes"] == nodes.tolist() and got["dist"] == dist.tolist()
        assert got["evals"] == walker.evals.value - e0
        assert got["longest"] <= ef and not got["cut"]


def test_fewer_passing_nodes_than_ef_returns_every_reachable_passing_node(graph, queries):
    passing = np.zeros(N, bool)
    chosen = [5, 31, 32, 700, 1999]
    passing[chosen] = True
    # cap above the node count: nothing is ever cut, the window never closes, so the walk visits the whole (connected) graph
    got = filtered_walk(graph, COS, queries[0], 10, 4096, passing)
    assert sorted(got["nodes"]) == chosen and got["longest"] == N and not got["cut"]
    assert got["dist"] == sorted(got["dist"])
    assert got["evals"] >= N
    # at a real capacity the list is cut (non-passing entries fall off its end) and the passing ones found are a subset
    small = filtered_walk(graph, COS, queries[0], 10, 64, passing)
    assert small["cut"] and small["longest"] == 64 and set(small["nodes"]) <= set(chosen)


def test_the_window_cut_keeps_exactly_ef_passing_entries_and_k_truncates(graph, queries):
    rng = np.random.default_rng(2002)
    passing = rng.random(N) < 0.25
    for q in queries[:4]:
        got = filtered_walk(graph, COS, q, 10, 512, passing)
        assert len(got["nodes"]) == 10 and all(passing[v] for v in got["nodes"])
        assert got["dist"] == sorted(got["dist"])
        assert 10 <= got["longest"] <= 512
        top3 = filtered_walk(graph, COS, q, 10, 512, passing, k=3)
        assert top3["nodes"] == got["nodes"][:3] and top3["evals"] == got["evals"]
        # the walk is a real search: what it returns is close to the exact nearest passing rows
        exact = np.argsort(-(graph["rows"][passing] @ q), kind="stable")[:10]
        truth = set(np.flatnonzero(passing)[exact].tolist())
        assert len(truth & set(got["nodes"])) >= 7


def test_an_entry_that_does_not_pass_still_navigates(graph, queries):
    passing = np.ones(N, bool)
    passing[0] = False  # the entry node (and, for a query next to it, the landing node of the descent)
    q = graph["rows"][0]
    got = filtered_walk(graph, COS, q, 5, 64, passing)
    assert 0 not in got["nodes"] and len(got["nodes"]) == 5
    everyone = filtered_walk(graph, COS, q, 6, 64, np.ones(N, bool))
    assert everyone["nodes"][0] == 0 and got["nodes"] == everyone["nodes"][1:]
