"""Grouped search (vl_index_search_grouped: the best row of each of the best k groups) against the oracle.  The expected
answer is the contract restated in Python: S = the rows that have a group (and pass the filter) in storage order,
oracle.FlatOracle over S gives the ranking, a loop keeps the first row of each group.  Group keys, ids and score bits are
compared with == for every query."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COS, EUC, MAN, DOT = 0, 1, 2, 3
METRICS = (COS, EUC, MAN, DOT)
K_FAST = (1, 10, 64)
K_EXACT = (65, 200, 1024)
GROUP_VARIANT_BASE = 5_000_000


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


def random_ids(rng, n):
    base = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(rng.integers(1 << 20))) % np.uint64(1 << 40)
    return rng.permutation(base)


def unit_rows(rng, n, dim):
    rows = rng.standard_normal((n, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    return np.ascontiguousarray(rows)


def clustered(rng, n, dim):
    """a few hundred centres plus small noise; returns the rows and each row's centre (cluster = group)"""
    centres = rng.standard_normal((min(300, max(1, n // 16)), dim))
    which = rng.integers(centres.shape[0], size=n)
    rows = centres[which] + 0.05 * rng.standard_normal((n, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    return np.ascontiguousarray(rows), which


def group_key(g):
    """dense numbers -> scattered u64 keys (0 and 2^64 - 1 among them)"""
    g = np.asarray(g, dtype=np.uint64)
    k = g * np.uint64(0x9E3779B97F4A7C15) + np.uint64(12345)
    k[g == 0] = np.uint64(0)
    k[g == 1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return k


class Case:
    """An index and its rows; gkeys[p] / has[p]: the group key of the row at storage position p and whether it has one."""

    def __init__(self, V, O, dim, ids, rows, gkeys, has=None):
        self.V, self.O, self.dim = V, O, dim
        self.ids = np.ascontiguousarray(ids, dtype=np.uint64)
        self.rows = np.ascontiguousarray(rows, dtype=np.float64)
        self.gkeys = np.ascontiguousarray(gkeys, dtype=np.uint64)
        self.has = np.ones(self.ids.size, dtype=bool) if has is None else np.asarray(has, dtype=bool)
        self.idx = V.FlatIndex(dim)
        self.idx.add_rows(self.ids, self.rows, validate=False)
        order = np.random.default_rng(7).permutation(int(self.has.sum()))  # the table's pairs in any order
        self.table = self.idx.make_groups(self.ids[self.has][order], self.gkeys[self.has][order])
        self._answers = {}

    def _subindex(self, allowed):
        """S in storage order and the oracle holding it (ids = storage positions); one per filter, shared by its queries"""
        key = None if allowed is None else allowed.tobytes()
        refs = self.__dict__.setdefault("_refs", {})
        if key not in refs:
            member = self.has if allowed is None else (self.has & allowed)
            positions = np.nonzero(member)[0].astype(np.uint64)
            ref = self.O.FlatOracle(self.dim, positions, self.rows[positions.astype(np.int64)]) if positions.size else None
            refs[key] = (positions, ref)
        return refs[key]

    def answer(self, q, metric, allowed=None):
        """the whole collapsed ranking (keys, ids, scores) for one query: computed once, every k is a prefix of it"""
        key = (q.tobytes(), metric, None if allowed is None else allowed.tobytes())
        hit = self._answers.get(key)
        if hit is None:
            positions, ref = self._subindex(allowed)
            keys, ids, scores = [], [], []
            if positions.size:
                rp, rs = ref.search(q, positions.size, metric)
                seen = set()
                for p, s in zip(rp.tolist(), rs.tolist()):
                    g = int(self.gkeys[p])
                    if g not in seen:
                        seen.add(g)
                        keys.append(g)
                        ids.append(int(self.ids[p]))
                        scores.append(s)
            hit = (keys, ids, bits(scores))
            self._answers[key] = hit
        return hit

    def check(self, q, k, metric, filt=None, allowed=None, tag=None):
        ek, ei, es = self.answer(q, metric, allowed)
        gk, gi, gs = self.idx.search_grouped_arrays(q, k, metric, groups=self.table, filter=filt)
        assert gk.tolist() == ek[:k], (tag, metric, k)
        assert gi.tolist() == ei[:k], (tag, metric, k)
        assert bits(gs) == es[:k], (tag, metric, k)
        return len(ek)


def make_case(V, O, shape, dim, n, seed):
    rng = np.random.default_rng(seed)
    ids = random_ids(rng, n)
    has = None
    if shape == "one_per_group":
        rows, g = unit_rows(rng, n, dim), np.arange(n)
    elif shape == "eight_per_group":
        rows, g = unit_rows(rng, n, dim), rng.integers(max(n // 8, 64), size=n)
    elif shape == "clustered":
        rows, g = clustered(rng, n, dim)
    else:  # "partial": 60 % of the ids have a group, ~8 rows per group
        rows, g = unit_rows(rng, n, dim), rng.integers(max(n // 8, 64), size=n)
        has = rng.random(n) < 0.6
    return Case(V, O, dim, ids, rows, group_key(g), has), rng


def queries_for(case, rng, shape, count=4):
    n = case.ids.size
    if shape == "clustered":  # a question about one of the rows: its best 64 rows lie in one or two clusters
        return [case.rows[rng.integers(n)] + 0.02 * rng.standard_normal(case.dim) for _ in range(count)]
    if shape == "partial":    # aimed at rows WITHOUT a group: they score best and must never appear
        out = np.nonzero(~case.has)[0]
        return [case.rows[out[rng.integers(out.size)]] + 0.02 * rng.standard_normal(case.dim) for _ in range(count)]
    return [rng.standard_normal(case.dim) for _ in range(count)]


# ---- 1. parity, both routes ----------------------------------------------------------------------
# dim 384: a specialised stride, the query in the kernel arguments; 1024: a specialised stride, the f64 query form (above 768
# floats); 32 and 100: the run-time-stride kernel (8 and 25 float4 per row are not among VL_SCAN_VARIANTS)
@pytest.mark.parametrize("shape", ["one_per_group", "eight_per_group", "clustered", "partial"])
@pytest.mark.parametrize("dim", [32, 100, 384, 1024])
def test_parity_with_the_restated_contract(V, O, dim, shape):
    n = 3000 if dim == 1024 else 5000
    case, rng = make_case(V, O, shape, dim, n, 100 * dim + len(shape))
    ungrouped_ids = set(case.ids[~case.has].tolist())
    for metric in METRICS:
        for q in queries_for(case, rng, shape):
            distinct = len(case.answer(q, metric)[0])
            assert distinct >= 64  # the oracle's own ranking holds 64 groups: the fast route can answer k = 64
            for k in K_FAST:
                case.check(q, k, metric, tag=(dim, shape))
                assert V.last_path() == V.PATH_FAST, (dim, shape, metric, k)
                variant = case.idx.last_scan()["variant"]
                if dim in (32, 100):
                    assert -(GROUP_VARIANT_BASE + 64) <= variant <= -(GROUP_VARIANT_BASE + 1)
                else:
                    assert GROUP_VARIANT_BASE < variant < GROUP_VARIANT_BASE + 1_000_000
                    if dim == 384:
                        assert variant == GROUP_VARIANT_BASE + 8 * 10000 + 12 * 100 + 1
            for k in K_EXACT:
                case.check(q, k, metric, tag=(dim, shape))
                assert V.last_path() == V.PATH_EXACT_SORT, (dim, shape, metric, k)
            gk, gi, _ = case.idx.search_grouped_arrays(q, 64, metric, groups=case.table)
            assert not (set(gi.tolist()) & ungrouped_ids)
            if shape == "clustered":  # what a plain top-64 would have shown: a handful of groups
                top_rows = case.O.FlatOracle(dim, np.arange(n, dtype=np.uint64), case.rows).search(q, 64, metric)[0]
                assert len(set(case.gkeys[top_rows.astype(np.int64)].tolist())) < 64


def test_a_grid_of_many_waves_races_on_best(V, O):
    """70 000 rows at dim 384: more steps than waves, so rows of one group are scored by different waves at the same time"""
    case, rng = make_case(V, O, "eight_per_group", 384, 70_000, 4242)
    for metric in METRICS:
        for q in queries_for(case, rng, "eight_per_group"):
            for k in K_FAST:
                case.check(q, k, metric)
                assert V.last_path() == V.PATH_FAST
    q = rng.standard_normal(384)
    case.check(q, 200, COS)
    assert V.last_path() == V.PATH_EXACT_SORT


# dim 128 and 256: specialised strides whose default shapes keep U = 3 and U = 2 row groups in flight per wave, so the sink's
# batched group-number loads, slot loads and conditional atomics run with more than one entry
@pytest.mark.parametrize("dim,shape_code", [(128, 8 * 10000 + 4 * 100 + 3), (256, 8 * 10000 + 8 * 100 + 2)])
def test_shapes_with_several_row_groups_in_flight(V, O, dim, shape_code):
    for shape in ("eight_per_group", "partial"):
        case, rng = make_case(V, O, shape, dim, 5000, 9 * dim + len(shape))
        for metric in METRICS:
            for q in queries_for(case, rng, shape):
                assert len(case.answer(q, metric)[0]) >= 64
                for k in K_FAST:
                    case.check(q, k, metric, tag=(dim, shape))
                    assert V.last_path() == V.PATH_FAST, (dim, shape, metric, k)
                    assert case.idx.last_scan()["variant"] == GROUP_VARIANT_BASE + shape_code
        with case.idx.make_filter(case.ids[::3]) as f:  # the listed-rows form of the same shape
            allowed = np.zeros(case.ids.size, dtype=bool)
            allowed[::3] = True
            for q in queries_for(case, rng, shape):
                case.check(q, 10, COS, filt=f, allowed=allowed)
                assert V.last_path() == V.PATH_FAST
                assert case.idx.last_scan()["variant"] == GROUP_VARIANT_BASE + shape_code


def test_more_survivors_than_the_speculative_ranking_holds(V, O):
    """80 groups of 100 near-identical rows: the rows scoring at least L (64 groups' worth) are more than the 2048 the
    tail ranks before the host knows their number, so the fast route ranks and collapses a second time."""
    rng = np.random.default_rng(2048)
    dim, groups, per = 384, 80, 100
    n = groups * per
    centres = unit_rows(rng, groups, dim)
    which = rng.permutation(np.repeat(np.arange(groups), per))
    rows = centres[which] + 0.002 * rng.standard_normal((n, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    case = Case(V, O, dim, random_ids(rng, n), np.ascontiguousarray(rows), group_key(which))
    for metric in METRICS:
        for q in [rng.standard_normal(dim) for _ in range(4)]:
            positions, ref = case._subindex(None)
            rs = ref.search(q, n, metric)[1]
            ek, _, es = case.answer(q, metric)
            L = np.array(es[63], dtype=np.uint64).view(np.float64)
            assert int((rs >= L).sum()) > 2048  # the case is what it says
            for k in (10, 64):
                case.check(q, k, metric)
                assert V.last_path() == V.PATH_FAST, (metric, k)
            case.check(q, 80, metric)
            assert V.last_path() == V.PATH_EXACT_SORT


# ---- 2. ties --------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_planted_ties(V, O, metric):
    rng = np.random.default_rng(31 + metric)
    n, dim, k = 4000, 32, 10
    ids = random_ids(rng, n)
    rows = unit_rows(rng, n, dim)
    g = np.arange(n)  # one row per group, then edited
    q = rng.standard_normal(dim)
    rp = O.FlatOracle(dim, np.arange(n, dtype=np.uint64), rows).search(q, n, metric)[0].astype(np.int64)
    tail = np.sort(rp[2000:])       # rows far from the top: their slots receive the copies
    # the k-th group's row copied into a LOWER and a HIGHER position of two other groups: a three-way tie across the k-th
    # place, ordered by position
    r = int(rp[k - 1])
    lo, hi = int(tail[tail < r][0]), int(tail[tail > r][-1])
    rows[lo] = rows[r]
    rows[hi] = rows[r]
    # bit-identical rows in the SAME group: the third-best row copied into a lower position that joins its group
    r3 = int(rp[2])
    lo3 = int(tail[(tail < r3) & (tail != lo)][0])
    rows[lo3] = rows[r3]
    g[lo3] = g[r3]
    case = Case(V, O, dim, ids, rows, group_key(g))
    ek, ei, _ = case.answer(q, metric)
    assert ei[2] == int(ids[lo3])                                        # the lower position shows the group
    assert ei[k - 1:k + 2] == [int(ids[lo]), int(ids[r]), int(ids[hi])]  # position order across the k-th place
    for kk in (3, k - 1, k, k + 1, k + 2, 64):
        case.check(q, kk, metric)
        assert V.last_path() == V.PATH_FAST
    for kk in (65, 1024):
        case.check(q, kk, metric)
        assert V.last_path() == V.PATH_EXACT_SORT
    case.idx.force_path(V.PATH_EXACT_SORT)
    try:
        case.check(q, k, metric)
        assert V.last_path() == V.PATH_EXACT_SORT
    finally:
        case.idx.force_path(0)


# ---- 3. few groups, empty S, NaN ------------------------------------------------------------------
def test_fewer_groups_than_k_empty_tables_and_nan(V, O):
    rng = np.random.default_rng(5)
    n, dim = 3000, 32
    ids = random_ids(rng, n)
    rows = unit_rows(rng, n, dim)
    case = Case(V, O, dim, ids, rows, group_key(rng.integers(5, size=n)))
    q = rng.standard_normal(dim)
    for metric in METRICS:
        assert case.check(q, 10, metric) == 5
        assert V.last_path() == V.PATH_EXACT_SORT  # fewer than k groups have a row
        gk, _, _ = case.idx.search_grouped_arrays(q, 10, metric, groups=case.table)
        assert len(gk) == 5
        case.check(q, 5, metric)
        assert V.last_path() == V.PATH_FAST
    assert case.table.rows() == n and case.table.distinct() == 5
    # a table none of whose ids the index holds: S is empty; the dimension check still runs
    with case.idx.make_groups([1 << 50, (1 << 50) + 1], [3, 4]) as t:
        assert t.rows() == 0 and t.distinct() == 2
        gk, gi, gs = case.idx.search_grouped_arrays(q, 10, COS, groups=t)
        assert gk.size == 0 and gi.size == 0 and gs.size == 0
        assert V.last_path() == V.PATH_NONE  # no scan ran: not the previous call's route
        with pytest.raises(V.DimensionMismatch):
            case.idx.search_grouped_arrays(np.zeros(7), 10, COS, groups=t)
    with case.idx.make_groups([], []) as t:
        assert case.idx.search_grouped_arrays(q, 10, COS, groups=t)[0].size == 0
    assert case.idx.search_grouped_arrays(q, 0, COS, groups=case.table)[0].size == 0
    with pytest.raises(V.IndexOpError, match="two different group keys"):
        case.idx.make_groups([1, 2, 1], [5, 5, 6])
    with pytest.raises(V.IndexOpError, match="VL_GROUPED_MAX_K"):
        case.idx.search_grouped_arrays(q, 1025, COS, groups=case.table)
    with pytest.raises(V.IndexOpError):
        case.idx.search_grouped_arrays(q, 10, 9, groups=case.table)  # unknown metric
    assert V.FlatIndex(8).make_groups([1], [1]).rows() == 0

    # NaN rows: one of them alone in S is returned whatever it scores, two of them fail like the reference's sort
    rows2 = rows.copy()
    rows2[10, 0] = np.nan
    rows2[20, 3] = np.nan
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows2, validate=False)
    with idx.make_groups([ids[10]], [77]) as t:
        gk, gi, gs = idx.search_grouped_arrays(q, 10, COS, groups=t)
        assert gk.tolist() == [77] and gi.tolist() == [int(ids[10])] and np.isnan(gs[0])
    with idx.make_groups([ids[10], ids[20]], [77, 78]) as t:
        with pytest.raises(V.NaNScore):
            idx.search_grouped_arrays(q, 10, COS, groups=t)
    with idx.make_groups([ids[10], ids[30]], [77, 78]) as t:
        with pytest.raises(V.NaNScore):
            idx.search_grouped_arrays(q, 1, COS, groups=t)
    # NaN rows outside S do not matter: not in the table, or kept out by the filter
    clean = np.ones(n, dtype=bool)
    clean[[10, 20]] = False
    ref = Case.__new__(Case)
    ref.V, ref.O, ref.dim, ref.ids, ref.rows = V, O, dim, ids, rows2
    ref.gkeys, ref.has, ref.idx, ref._answers, ref._refs = case.gkeys, clean, idx, {}, {}
    ref.table = idx.make_groups(ids[clean], case.gkeys[clean])
    ref.check(q, 5, COS)
    assert V.last_path() == V.PATH_EXACT_SORT  # rows outside the fast-path domain
    full = idx.make_groups(ids, case.gkeys)
    ref.has, ref.table, ref._answers, ref._refs = np.ones(n, dtype=bool), full, {}, {}
    with idx.make_filter(ids[clean]) as f:
        ref.check(q, 5, COS, filt=f, allowed=clean)
    with pytest.raises(V.NaNScore):
        idx.search_grouped_arrays(q, 5, COS, groups=full)


# ---- 4. id filters --------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [0.01, 0.3, 1.0])
def test_with_an_id_filter_the_answer_is_the_intersections(V, O, share):
    case, rng = make_case(V, O, "partial", 384, 6000, 77)
    n = case.ids.size
    allowed = np.ones(n, dtype=bool) if share == 1.0 else rng.random(n) < share
    with case.idx.make_filter(case.ids[allowed]) as f:
        for metric in METRICS:
            for q in queries_for(case, rng, "partial"):
                for k in (1, 10, 64, 200):
                    distinct = case.check(q, k, metric, filt=f, allowed=allowed)
                    want = V.PATH_FAST if k <= min(64, distinct) else V.PATH_EXACT_SORT
                    assert V.last_path() == want, (share, metric, k, distinct)
        # a one-shot filter given as ids
        q = rng.standard_normal(384)
        ek, ei, es = case.answer(q, COS, allowed)
        gk, gi, gs = case.idx.search_grouped_arrays(q, 10, COS, groups=case.table, filter=case.ids[allowed])
        assert (gk.tolist(), gi.tolist(), bits(gs)) == (ek[:10], ei[:10], es[:10])
    n_out = C.c_uint64(3)  # an unknown filter token
    buf, sc = np.zeros(8, dtype=np.uint64), np.zeros(8)
    rc = case.idx._L.vl_index_search_grouped(case.idx._h, case.table.token, 987654321, q.ctypes.data, q.size, 4, COS, 8,
                                             buf.ctypes.data, buf.ctypes.data, sc.ctypes.data, C.byref(n_out))
    assert rc == 8 and n_out.value == 0


# ---- 5. capacity, prefixes, the Python surface ----------------------------------------------------
def test_capacity_prefix_and_result_objects(V, O):
    case, rng = make_case(V, O, "eight_per_group", 384, 5000, 909)
    q = rng.standard_normal(384)
    for metric in METRICS:
        ek, ei, es = case.answer(q, metric)
        k64 = case.idx.search_grouped_arrays(q, 64, metric, groups=case.table)
        k10 = case.idx.search_grouped_arrays(q, 10, metric, groups=case.table)
        for a, b in zip(k10, k64):
            assert a.view(np.uint64).tolist() == b[:10].view(np.uint64).tolist()
        for k, cap in ((10, 3), (64, 7), (200, 50), (10, 0)):
            keys = np.zeros(max(cap, 1), dtype=np.uint64)
            ids = np.zeros(max(cap, 1), dtype=np.uint64)
            sc = np.zeros(max(cap, 1))
            n_out = C.c_uint64(99)
            rc = case.idx._L.vl_index_search_grouped(case.idx._h, case.table.token, 0, q.ctypes.data, q.size, k, metric, cap,
                                                     keys.ctypes.data, ids.ctypes.data, sc.ctypes.data, C.byref(n_out))
            assert rc == 0 and n_out.value == cap
            assert keys[:cap].tolist() == ek[:cap] and ids[:cap].tolist() == ei[:cap] and bits(sc[:cap]) == es[:cap]
    res = case.idx.search_grouped(q, 5, V.SimilarityMetric.Cosine, groups=case.table)
    ek, ei, es = case.answer(q, COS)
    assert [g for g, _ in res] == ek[:5]
    assert [r.id for _, r in res] == ei[:5] and all(isinstance(r, V.SearchResult) for _, r in res)
    with pytest.raises(ValueError):
        case.idx.search_grouped_arrays(q, 5, COS)
    with pytest.raises(ValueError):
        V.FlatIndex(384).search_grouped_arrays(q, 5, COS, groups=case.table)


# ---- 6. candidate overflow -------------------------------------------------------------------------
_OVERFLOW_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import vectorlite_amd as V
from oracle import oracle as O
import test_gpu_grouped_search as T
case, rng = T.make_case(V, O, "eight_per_group", 384, 5000, 606)
paths = set()
for metric in (0, 1, 2, 3):
    for q in T.queries_for(case, rng, "eight_per_group"):
        for k in (1, 10, 64):
            case.check(q, k, metric)
            paths.add((k, V.last_path()))
assert (64, V.PATH_EXACT_SORT) in paths, paths  # 64 groups' rows and more pass the threshold: over the 64 slots
assert (1, V.PATH_FAST) in paths, paths
print("overflow-ok")
"""


def test_candidate_buffer_overflow_takes_the_exact_route(tmp_path):
    """With the candidate capacity lowered to 64 positions (a fresh process: the knob is the process's environment) the
    calls whose second pass keeps more rows take the exact route; the answers are the same."""
    script = tmp_path / "grouped_overflow_child.py"
    script.write_text(_OVERFLOW_CHILD)
    env = dict(os.environ, VL_RANGE_CAND_CAP="64")
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "overflow-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 7. the table follows the index ---------------------------------------------------------------
def test_the_table_follows_add_and_delete_and_tokens_are_the_handles(V, O):
    case, rng = make_case(V, O, "eight_per_group", 32, 3000, 11)
    idx, table, dim = case.idx, case.table, 32
    q = rng.standard_normal(dim)
    q /= np.linalg.norm(q)
    ek, ei, _ = case.answer(q, COS)
    assert table.rows() == 3000
    best_id, third_key = ei[0], ek[2]
    idx.delete(best_id)                                   # the best group loses its best row
    moved_id = int(case.ids[case.gkeys == np.uint64(third_key)][0])
    idx.delete(moved_id)
    idx.add(V.Vector(moved_id, q.tolist()))               # a grouped id comes back as the best row of all
    idx.add(V.Vector((1 << 41) + 5, q.tolist()))          # an id the table does not hold: no part, however good
    now_ids, now_rows = idx.export()
    key_of = dict(zip(case.ids.tolist(), case.gkeys.tolist()))
    after = Case.__new__(Case)
    after.V, after.O, after.dim, after.idx, after.table, after._answers = V, O, dim, idx, table, {}
    after.ids, after.rows = now_ids, np.ascontiguousarray(now_rows)
    after.has = np.array([i in key_of for i in now_ids.tolist()])
    after.gkeys = np.array([key_of.get(i, 0) for i in now_ids.tolist()], dtype=np.uint64)
    for metric in METRICS:
        for k in (1, 10, 64, 100):
            after.check(q, k, metric)
    gk, gi, _ = idx.search_grouped_arrays(q, 3, COS, groups=table)
    assert gi[0] == moved_id and gk[0] == third_key and best_id not in gi.tolist()
    assert table.rows() == 2999 and table.distinct() == len(set(case.gkeys.tolist()))

    twin = idx.clone()                                    # a clone does not know the token
    n_out = C.c_uint64(0)
    buf, sc = np.zeros(8, dtype=np.uint64), np.zeros(8)

    def raw(h, token):
        return idx._L.vl_index_search_grouped(h, token, 0, q.ctypes.data, q.size, 4, COS, 8, buf.ctypes.data, buf.ctypes.data,
                                              sc.ctypes.data, C.byref(n_out))
    assert raw(idx._h, table.token) == 0 and n_out.value == 4
    assert raw(twin._h, table.token) == 8 and n_out.value == 0
    token = table.token
    table.close()
    assert raw(idx._h, token) == 8 and n_out.value == 0  # a destroyed token
    assert idx._L.vl_index_groups_destroy(idx._h, token) == 8
    out = C.c_uint64(0)
    assert idx._L.vl_index_groups_rows(idx._h, token, C.byref(out), None) == 8
    with pytest.raises(V.IndexOpError):
        table.rows()


# ---- 8. concurrency --------------------------------------------------------------------------------
def test_eight_threads_two_tables_one_handle(V, O):
    case, rng = make_case(V, O, "eight_per_group", 384, 8000, 314)
    other = Case.__new__(Case)
    other.__dict__.update(case.__dict__)
    other.gkeys = group_key(rng.integers(200, size=case.ids.size))
    other.table, other._answers, other._refs = case.idx.make_groups(case.ids, other.gkeys), {}, {}
    qs = [rng.standard_normal(384) for _ in range(4)]
    for c in (case, other):  # the lone calls (and their references) first
        for q in qs:
            for k in (10, 64, 100):
                c.check(q, k, COS)
    errors = []

    def worker(t):
        try:
            c = case if t % 2 == 0 else other
            for rep in range(6):
                for q in qs:
                    c.check(q, (10, 64, 100)[(t + rep) % 3], COS, tag=("thread", t))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert errors == []


# ---- 9. handles that refuse ------------------------------------------------------------------------
def test_hnsw_and_multi_gpu_handles_refuse(V):
    rng = np.random.default_rng(2)
    q = rng.standard_normal(8)
    hn = V.HNSWIndex(8)
    hn.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        hn.make_groups([1, 2], [1, 1])
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        hn.search_grouped_arrays(q, 3, COS)
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        hn.search_grouped(q, 3, COS)
    mi = V.MultiFlatIndex(8, [0, 0])
    mi.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        mi.make_groups([1, 2], [1, 1])
    n_out = C.c_uint64(5)
    buf, sc = np.zeros(8, dtype=np.uint64), np.zeros(8)
    for h in (hn._h, mi._h):
        rc = mi._L.vl_index_search_grouped(h, 1, 0, q.ctypes.data, q.size, 3, COS, 8, buf.ctypes.data, buf.ctypes.data,
                                           sc.ctypes.data, C.byref(n_out))
        assert rc == 8 and n_out.value == 0
