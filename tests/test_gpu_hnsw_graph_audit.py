"""Audit of the HNSW graph the batched GPU build leaves behind, and the full-beam property of both walks (HNSW
section).

tests/native/hnsw_graph_audit.hip drives HnswIndex in C++.  After every mutation it copies the graph arrays, the row slab
and the host bookkeeping back and runs tests/native/hnsw_graph_check.hpp on them (G1 .. G8: the level law, entry point,
list bounds and levels, no node named twice, every stored edge distance the build's f32 key as bits, the in-degree counter,
locks and tails at rest, the id maps; G9 reachability reported), then V1: every walk scratch idle, every visited bit zero.
  a  boundaries: 40 single adds from empty, growth across 1024 and 2048, bulk adds of 1 / 2 / 17 rows, two refused bulk
     adds, ten deletes; 60 copies of one row and zero rows among them (euclidean dim 5, cosine dim 100)
  b  (m, m0) = (4, 8) on 2000 clustered rows and (48, 64) on 600 rows, manhattan and dot product, five uneven bulk adds
  c  ef_construction 64 / 128 / 256 / 512, a clone, 50 rows added to the clone only
  d  40 000 rows of dim 64 in one bulk add (the 4096-node batch cap), two batches of 64 walks at ef = 512 whose visited
     logs overflow: measured 9315.0 evaluations per query (the stream fails at or below 8192 + 513: a walk's evaluations
     are the nodes it marked, the entry point and the 512 re-scorings of its beam).  i.i.d. rows of dim 8 / 16 / 32 gave
     3666 / 7301 (at 100 000 rows) / 8512: the lower the dimension the more the beam's neighbourhoods overlap
  e  8 host threads walking at once without coalescing; every answer equals the one the same call gives alone
A path from the entry point to every node (G9) is demanded up to m0 + 1 nodes, where the build guarantees it, and counted
beyond: the build promises every node an incoming edge, and two nodes can hold each other's last one (measured in stream a:
2 of 2060 euclidean dim-5 nodes, naming each other only).  With lists of 8 not even the incoming edge can be promised
(measured: 13 of 2000 nodes without one under the dot product); it is refused everywhere else.

The full-beam tests are in Python: with ef >= the number of nodes nothing is ever rejected from the beam, so a walk returns
exactly the nodes reachable on layer 0 from where its descent lands, whatever f32 rounding did on the way.
"""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def audit_exe(tmp_path_factory):
    from vectorlite_amd import build as vbuild
    vbuild.build()  # the program links the library's objects: the private members the probe reads
    d = tmp_path_factory.mktemp("hnsw_graph_audit")
    exe, obj = d / "hnsw_graph_audit", d / "hnsw_graph_audit.o"
    arch = [vbuild.hipcc(), f"--offload-arch={vbuild.ARCH}"]
    objs = [os.path.join(vbuild.OBJ, os.path.splitext(s)[0] + ".o") for s in vbuild.SOURCES]
    for cmd in (arch + ["-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "hnsw_graph_audit.hip"), "-o", str(obj)],
                arch + [str(obj)] + objs + vbuild.LINK + ["-o", str(exe)]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


_STATE = {"failed_child": None}


def run_child(args, timeout):
    """One audit child; after a child that did not exit cleanly no further one is started (the link kernel spins on
    locks: a child that reaches its time limit has hung and is not to be run again before the cause is found)."""
    if _STATE["failed_child"]:
        pytest.fail(f"not started: the audit child {_STATE['failed_child']} failed")
    _STATE["failed_child"] = " ".join(args[1:])
    r = subprocess.run(args, capture_output=True, text=True, timeout=timeout)
    if r.returncode == 0 and "audit ok" in r.stdout:
        _STATE["failed_child"] = None
    else:
        pytest.fail(f"audit child exited {r.returncode}:\n{r.stdout[-6000:]}\n{r.stderr[-3000:]}")
    return r.stdout


def summary_lines(out):
    return [l for l in out.splitlines() if l.startswith("stream ")]


def checkpoints(line):
    return int(line.split(":")[1].split()[0])


def test_a_boundaries(audit_exe):
    out = run_child([audit_exe, "a"], timeout=120)
    lines = summary_lines(out)
    print("\n" + "\n".join(lines))
    assert len(lines) == 2 and "dim=5 " in lines[0] and "dim=100 " in lines[1], out[-2000:]
    # empty + 40 single adds + 2 bulk adds across a capacity step + bulk adds of 1, 2, 17 + 2 refused + 10 deletes
    assert [checkpoints(l) for l in lines] == [58, 58], lines
    # every node keeps an incoming edge; a path from the entry point is demanded by the program up to m0 + 1 nodes, where
    # the build guarantees it, and the count is printed beyond (two nodes can hold each other's last edge)
    assert all("orphans_max=0 " in l for l in lines), lines


def test_b_small_and_large_lists(audit_exe):
    out = run_child([audit_exe, "b"], timeout=120)
    lines = summary_lines(out)
    print("\n" + "\n".join(lines))
    assert len(lines) == 4 and [checkpoints(l) for l in lines] == [5, 5, 5, 5], out[-2000:]
    assert sum("m=4 m0=8 " in l for l in lines) == 2 and sum("m=48 m0=64 " in l for l in lines) == 2, lines
    # lists of 8 cannot promise every node an incoming edge: counted there, refused at m0 = 64
    assert all("orphans_max=0 " in l for l in lines if "m0=64 " in l), lines


def test_c_the_four_beam_shapes_of_the_build_and_clones(audit_exe):
    out = run_child([audit_exe, "c"], timeout=120)
    lines = summary_lines(out)
    print("\n" + "\n".join(lines))
    assert len(lines) == 4 and [checkpoints(l) for l in lines] == [4, 4, 4, 4], out[-2000:]
    assert [l.split("ef_construction=")[1].split()[0] for l in lines] == ["64", "128", "256", "512"], lines
    assert all("orphans_max=0 " in l for l in lines), lines


def test_d_the_big_batch_and_the_visited_log_overflow(audit_exe):
    out = run_child([audit_exe, "d"], timeout=120)
    lines = summary_lines(out)
    print("\n" + "\n".join(lines))
    assert len(lines) == 1 and checkpoints(lines[0]) == 3, out[-2000:]
    assert float(lines[0].split("evals_per_query=")[1].split()[0]) > 8192.0, lines


def test_e_concurrent_walkers(audit_exe):
    out = run_child([audit_exe, "e"], timeout=120)
    lines = summary_lines(out)
    print("\n" + "\n".join(lines))
    assert len(lines) == 1 and checkpoints(lines[0]) == 3, out[-2000:]


# ---- the full-beam property ------------------------------------------------------------------------------------------
METRICS = (0, 1, 2, 3)  # cosine, euclidean, manhattan, dot
SHAPES = ((40, 64), (100, 128), (200, 256), (500, 512))  # (nodes, ef): one per list shape of BeamList (1, 2, 4, 8 entries a lane)
NQ = 16


def _keys(metric, Q, X):
    """[nq, n] walk keys: Metric::distance's f64 value before `as u64`, accumulated in index order with a separate
    multiply and add (numpy rounds every elementwise operation on its own), negative values and NaN at 0 as the cast puts
    them.  trunc(key) is checked against the oracle's u64 by the caller."""
    nq, n, dim = Q.shape[0], X.shape[0], X.shape[1]
    a = np.zeros((nq, n))
    b = np.zeros((nq, n))
    c = np.zeros((nq, n))
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


class _Cell:
    """One index with everything the full-beam checks need, computed once."""

    def __init__(self, V, O, metric, dim, n, m=16, m0=32, seed=0):
        rng = np.random.default_rng(1000 * metric + dim + n + m)
        self.metric, self.n = metric, n
        self.X = rng.standard_normal((n, dim))
        self.Q = rng.standard_normal((NQ, dim))
        self.ids = np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(3)
        self.idx = V.HNSWIndex(dim, metric, m=m, m0=m0, seed=seed)  # the default ef_construction
        self.idx.add_rows(self.ids, self.X)
        self.refresh(O)
        self.keys = _keys(metric, self.Q, self.X)
        self.u64 = np.array([[O.hnsw_distance(metric, self.Q[i], self.X[j]) for j in range(n)] for i in range(NQ)], dtype=np.uint64)
        assert (np.floor(self.keys).astype(np.uint64) == self.u64).all()  # the restated key is the oracle's distance before the cast
        self.score = {int(d): O.hnsw_score(int(d), metric) for d in np.unique(self.u64)}

    def refresh(self, O):
        g = self.idx.graph(with_rows=True)
        self.g = g
        self.adj = [g["nbr0"][i, :int(g["cnt0"][i])].tolist() for i in range(self.n)]
        self.rev = [[] for _ in range(self.n)]
        for i, l in enumerate(self.adj):
            for e in l:
                self.rev[e].append(i)
        self.strong = bool(_flood(self.adj, 0, self.n).all() and _flood(self.rev, 0, self.n).all())
        self.walker = O.HnswCpuWalker(g, self.metric)

    def reachable_set_matching(self, nodes):
        """The node whose layer-0 reachable set is exactly `nodes` (None: no node has that set)."""
        want = np.zeros(self.n, bool)
        want[list(nodes)] = True
        for v in nodes:
            if (_flood(self.adj, v, self.n) == want).all():
                return v
        return None


def _check_cell(cell, ef, dead=(), explicit_ef=True):
    """Both navigation modes at k = n.  Returns the per-mode answers (ids as node indexes)."""
    n, metric = cell.n, cell.metric
    live = np.ones(n, bool)
    live[list(dead)] = False
    out = {}
    for mode in ("f32", "reference"):
        cell.idx.set_navigation(mode)
        ids, scores, cnt = cell.idx.search_batch(cell.Q, n, metric, ef=ef if explicit_ef else 0)
        answers = []
        for i in range(NQ):
            c = int(cnt[i])
            nodes = ((ids[i, :c] - np.uint64(3)) // np.uint64(7)).astype(np.int64)
            assert (cell.ids[nodes] == ids[i, :c]).all()
            answers.append(nodes)
            # every score is the oracle's conversion of the oracle's u64 distance, as bits
            assert scores[i, :c].tolist() == [cell.score[int(cell.u64[i, v])] for v in nodes], (mode, i)
            assert live[nodes].all(), (mode, i)
            if not explicit_ef:
                continue  # judged against the explicit-ef answer by the caller
            # the set: every live node when layer 0 is strongly connected; otherwise the whole reachable set of some node,
            # the one the descent landed on or one that reaches the same nodes (only judged without tombstones)
            if cell.strong:
                walked = set(range(n))
            else:
                assert not dead
                walked = set(nodes.tolist())
                v = cell.reachable_set_matching(sorted(walked))
                print(f"metric {metric} n {n} query {i} {mode}: layer 0 is not strongly connected; the walk returned "
                      f"{len(walked)} nodes, the reachable set of node {v}")
                assert v is not None, (mode, i, len(walked))
            expected = np.array(sorted(v for v in walked if live[v]), dtype=np.int64)
            assert sorted(nodes.tolist()) == expected.tolist(), (mode, i, c, len(expected))
            if mode == "f32":
                # (exact f64 distance, node index): the u64 order with its ties broken by the true distance
                order = expected[np.lexsort((expected, cell.keys[i, expected]))]
                assert nodes.tolist() == order.tolist(), (mode, i)
            else:
                # the reference's u64 order; tied u64 values stay in the walker's first-seen order
                d = cell.u64[i, nodes]
                assert (d[1:] >= d[:-1]).all(), (mode, i)
                beam, _ = cell.walker.search(cell.Q[i], ef, n)
                assert nodes.tolist() == [int(v) for v in beam if live[int(v)]], (mode, i)
        out[mode] = answers
    cell.idx.set_navigation("f32")
    return out


@pytest.fixture(scope="module")
def VO():
    import vectorlite_amd as V
    from oracle import oracle as O
    O.build()
    return V, O


@pytest.mark.parametrize("dim", (7, 384))
@pytest.mark.parametrize("metric", METRICS)
def test_a_full_beam_returns_exactly_the_reachable_nodes_in_exact_order(VO, metric, dim):
    V, O = VO
    for n, ef in SHAPES:
        cell = _Cell(V, O, metric, dim, n)
        _check_cell(cell, ef)  # layer 0 should be strongly connected at these sizes; if not, _check_cell says what it saw


@pytest.mark.parametrize("metric", METRICS)
def test_a_full_beam_with_tombstones(VO, metric):
    V, O = VO
    for (n, ef), dim in zip(SHAPES, (7, 384, 7, 384)):
        cell = _Cell(V, O, metric, dim, n)
        assert cell.strong, (metric, dim, n)
        dead = [0, 1, n // 2, n - 2, n - 1]  # the first entry point among them
        for v in dead:
            cell.idx.delete(int(cell.ids[v]))
        # a caller that names its ef gets the freed slots refilled: the live nodes, in order
        full = _check_cell(cell, ef, dead=dead, explicit_ef=True)
        assert all(len(a) == n - 5 for mode in full for a in full[mode]), (metric, n)
        # no ef: the strict beam ef = min(k, len) = n - 5 over n nodes.  Until the beam is full nothing is rejected and
        # every entry is expanded, so on a strongly connected layer 0 it does fill: it ends with exactly n - 5 nodes, the
        # tombstones among THEM are dropped and nothing refills them.  Which of the farthest nodes the full beam turned
        # away is the f32 navigation's business, so the answer is the one above with at most 5 more nodes missing, in the
        # same order -- between n - 10 and n - 5 nodes
        strict = _check_cell(cell, ef, dead=dead, explicit_ef=False)
        for mode in strict:
            for a, b in zip(strict[mode], full[mode]):
                it = iter(b.tolist())
                assert all(v in it for v in a.tolist()), (mode, metric, n)  # same order
                print(f"metric {metric} n {n} {mode}: strict beam returned {len(a)} of {n - 5} live nodes")
                assert n - 10 <= len(a) <= n - 5, (mode, metric, n, len(a))


@pytest.mark.parametrize("m,m0", ((4, 8), (48, 64)))
@pytest.mark.parametrize("metric", METRICS)
def test_a_full_beam_on_short_and_long_lists(VO, metric, m, m0):
    V, O = VO
    cell = _Cell(V, O, metric, 7, 200, m=m, m0=m0)
    assert int(cell.g["cnt0"].max()) <= m0
    if m0 == 64:
        assert int(cell.g["cnt0"].max()) > 32  # the second round of 32 neighbours runs
    _check_cell(cell, 256)
