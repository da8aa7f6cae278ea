"""Range search (vl_index_search_range) against the oracle: the answer is the longest prefix of
FlatIndex::search(q, len, metric) whose scores satisfy score >= min_score -- ids equal, f64 scores equal bit for bit,
`total` equal to its length.  The expected answer always comes from the oracle's full ranking, cut in Python."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, EUC, MAN, DOT = 0, 1, 2, 3
METRICS = (COS, EUC, MAN, DOT)
RANGE_VARIANT_BASE = 4_000_000
# k_scan's default (G, VPL, U) per row stride in floats (the first entry of each stride in VL_SCAN_VARIANTS)
DEFAULT_SHAPE = {128: (8, 4, 3), 256: (8, 8, 2), 384: (8, 12, 1), 512: (8, 16, 1), 768: (16, 12, 1), 1024: (16, 16, 1),
                 1536: (16, 24, 1)}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def ranking(ref, q, metric):
    """The oracle's full ranking (ids, scores): one per (index, query, metric) serves all its thresholds."""
    return ref.search(q, len(ref), metric)


def expected(rank, min_score):
    ri, rs = rank
    ok = rs >= min_score  # the IEEE comparison; the ranking is score-descending, so the passing rows are a prefix
    m = int(ok.sum())
    assert bool(ok[:m].all())
    return ri[:m], rs[:m]


def thresholds(rs):
    n = rs.size
    out = [-np.inf, np.inf, 0.0, -0.0]
    for r in (0, 9, 63, 64, 1000, n - 1):
        if 0 <= r < n:
            s = rs[r]
            out += [s, np.nextafter(s, np.inf), np.nextafter(s, -np.inf)]
    return out


def check(idx, rank, q, min_score, metric, filt=None, limit=None, tag=None):
    ei, es = expected(rank, min_score)
    gi, gs, total = idx.search_range_arrays(q, min_score, metric, filter=filt, limit=limit)
    want = ei.size if limit is None else min(ei.size, limit)
    assert total == ei.size, (tag, metric, min_score, total, ei.size)
    assert gi.tolist() == ei[:want].tolist(), (tag, metric, min_score)
    assert bits(gs) == bits(es[:want]), (tag, metric, min_score)
    return total


def build(V, O, dim, ids, rows):
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    return idx, O.FlatOracle(dim, ids, rows)


# ---- 1. parity -----------------------------------------------------------------------------------
ALL_SIZES = (1, 63, 64, 65, 10_000, 200_000)


# dim 3 and 50: strides outside VL_SCAN_VARIANTS (the generic form); dim 1000: a stride above the 768 kernel-argument floats
@pytest.mark.parametrize("dim,sizes", [(3, ALL_SIZES), (50, ALL_SIZES), (384, ALL_SIZES), (768, ALL_SIZES),
                                       (1000, (1, 65, 10_000)), (1024, (64, 10_000))])
@pytest.mark.parametrize("unit", [False, True])
def test_parity_at_thresholds_that_sit_on_scores(V, O, dim, sizes, unit):
    rng = np.random.default_rng(dim + (7 if unit else 0))
    for n in sizes:
        ids = random_ids(rng, n)
        rows = rng.standard_normal((n, dim))
        if unit:
            rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        idx, ref = build(V, O, dim, ids, rows)
        q = rng.standard_normal(dim)
        if unit:
            q /= np.linalg.norm(q)
        for metric in METRICS:
            rank = ranking(ref, q, metric)
            for t in thresholds(rank[1]):
                check(idx, rank, q, float(t), metric, tag=(dim, n, unit))


# ---- 2. ties -------------------------------------------------------------------------------------
def test_identical_rows_come_back_in_insertion_order(V, O):
    rng = np.random.default_rng(2)
    n, dim = 3000, 384
    ids = random_ids(rng, n)
    rows = np.tile(rng.standard_normal(dim), (n, 1))  # the reference's mock-embedding case
    idx, ref = build(V, O, dim, ids, rows)
    q = rng.standard_normal(dim)
    for metric in METRICS:
        rank = ranking(ref, q, metric)
        s = float(rank[1][0])
        assert bits(rank[1]) == [bits([s])[0]] * n
        gi, _, total = idx.search_range_arrays(q, s, metric)
        assert total == n and gi.tolist() == ids.tolist()
        assert check(idx, rank, q, float(np.nextafter(s, np.inf)), metric) == 0


def test_blocks_of_duplicates_across_wave_and_workgroup_boundaries(V, O):
    rng = np.random.default_rng(3)
    n, dim = 60_000, 384
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    q = rng.standard_normal(dim)
    twin = q * 2.0
    for lo, hi in ((5, 12), (60, 70), (250, 262), (1020, 1030), (30_000, 30_040), (n - 3, n)):
        rows[lo:hi] = twin
    idx, ref = build(V, O, dim, ids, rows)
    for metric in METRICS:
        rank = ranking(ref, q, metric)
        s = float(rank[1][0])
        total = check(idx, rank, q, s, metric)
        assert total >= 7 + 10 + 12 + 10 + 40 + 3
        check(idx, rank, q, float(rank[1][200]), metric)


# ---- 3. capacity ---------------------------------------------------------------------------------
def test_capacity_is_a_prefix_and_total_is_always_reported(V, O):
    rng = np.random.default_rng(4)
    n, dim = 20_000, 50
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    idx, ref = build(V, O, dim, ids, rows)
    q = rng.standard_normal(dim)
    for metric in (COS, EUC):
        rank = ranking(ref, q, metric)
        for total in (40, 5000):
            t = float(rank[1][total - 1])
            assert expected(rank, t)[0].size == total
            for cap in (0, 1, total - 1, total, total + 7):
                check(idx, rank, q, t, metric, limit=cap)
    # count only, NULL outputs, straight through the C ABI
    n_out, tot = C.c_uint64(9), C.c_uint64(9)
    rank = ranking(ref, q, COS)
    rc = idx._L.vl_index_search_range(idx._h, 0, q.ctypes.data, q.size, float(rank[1][99]), COS, None, None, 0,
                                      C.byref(n_out), C.byref(tot))
    assert (rc, n_out.value, tot.value) == (0, 0, 100)


# ---- 4. large totals -----------------------------------------------------------------------------
def test_large_totals_and_forced_exact_path(V, O):
    rng = np.random.default_rng(5)
    n, dim = 200_000, 384
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    idx, ref = build(V, O, dim, ids, rows)
    q = rng.standard_normal(dim)
    for metric in (COS, EUC):
        rank = ranking(ref, q, metric)
        for t in (float(rank[1][n // 2 - 1]), float(rank[1][n - 1])):
            total = check(idx, rank, q, t, metric)
            assert total >= n // 2
            assert V.last_path() == V.PATH_FAST
            idx.force_path(V.PATH_EXACT_SORT)
            try:
                check(idx, rank, q, t, metric)
                assert V.last_path() == V.PATH_EXACT_SORT
                check(idx, rank, q, float(rank[1][9]), metric)
            finally:
                idx.force_path(0)


_OVERFLOW_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import vectorlite_amd as V
from oracle import oracle as O
rng = np.random.default_rng(6)
n, dim = 30_000, 384
ids = np.arange(n, dtype=np.uint64) + np.uint64(5)
rows = rng.standard_normal((n, dim))
idx = V.FlatIndex(dim)
idx.add_rows(ids, rows, validate=False)
ref = O.FlatOracle(dim, ids, rows)
q = rng.standard_normal(dim)
for metric in (0, 1, 2, 3):
    ri, rs = ref.search(q, n, metric)
    for rank, path in ((99, V.PATH_FAST), (4999, V.PATH_EXACT_SORT), (n - 1, V.PATH_EXACT_SORT)):
        gi, gs, total = idx.search_range_arrays(q, float(rs[rank]), metric)
        m = int((rs >= rs[rank]).sum())
        assert total == m and gi.tolist() == ri[:m].tolist(), (metric, rank, total, m)
        assert gs.view(np.uint64).tolist() == rs[:m].view(np.uint64).tolist(), (metric, rank)
        assert V.last_path() == path, (metric, rank, V.last_path())
    with idx.make_filter(ids[::2]) as f:
        sub = O.FlatOracle(dim, ids[::2], rows[::2])
        si, ss = sub.search(q, n, metric)
        gi, gs, total = idx.search_range_arrays(q, float(ss[2999]), metric, filter=f)
        m = int((ss >= ss[2999]).sum())
        assert total == m and gi.tolist() == si[:m].tolist() and V.last_path() == V.PATH_EXACT_SORT
        assert gs.view(np.uint64).tolist() == ss[:m].view(np.uint64).tolist()
print("overflow-ok")
"""


def test_candidate_buffer_overflow_takes_the_exact_route(V, O, tmp_path):
    """With the candidate capacity lowered to 1000 positions (a fresh process: the knob is the process's environment),
    thresholds that let more rows through take the exact route and say so; the answer is the same."""
    script = tmp_path / "overflow_child.py"
    script.write_text(_OVERFLOW_CHILD)
    env = dict(os.environ, VL_RANGE_CAND_CAP="1000")
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "overflow-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 5. paths ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [100, 128, 384, 768, 1000, 1024])
def test_fast_path_and_the_scan_that_ran(V, O, dim):
    rng = np.random.default_rng(dim)
    n = 20_000
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    idx, ref = build(V, O, dim, ids, rows)
    q = rng.standard_normal(dim)
    ld = (dim + 3) & ~3
    for metric in METRICS:
        rank = ranking(ref, q, metric)
        check(idx, rank, q, float(rank[1][9]), metric)
        assert V.last_path() == V.PATH_FAST
        variant = idx.last_scan()["variant"]
        if ld in DEFAULT_SHAPE:
            g, vpl, u = DEFAULT_SHAPE[ld]
            assert variant == RANGE_VARIANT_BASE + g * 10000 + vpl * 100 + u
        else:
            assert -(RANGE_VARIANT_BASE + 64) <= variant <= -(RANGE_VARIANT_BASE + 1)  # the generic form, G lanes per row


# ---- 6. domain -----------------------------------------------------------------------------------
def test_rows_and_queries_outside_the_fast_path_domain(V, O):
    rng = np.random.default_rng(8)
    n, dim = 5000, 64
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    rows[17] = 0.0                       # a zero row: cosine 0.0
    q = rng.standard_normal(dim)
    idx, ref = build(V, O, dim, ids, rows)
    rank = ranking(ref, q, COS)
    for t in (0.0, -0.0):
        gi, _, _ = idx.search_range_arrays(q, t, COS)
        assert int(ids[17]) in gi.tolist()
        check(idx, rank, q, t, COS)
        assert V.last_path() == V.PATH_FAST
    for metric in METRICS:               # a query of zeros (cosine: every score is 0.0)
        z = np.zeros(dim)
        zr = ranking(ref, z, metric)
        for t in (0.0, float(zr[1][10]), float(np.nextafter(zr[1][0], np.inf)), -np.inf):
            check(idx, zr, z, t, metric)
    big = rows.copy()
    big[99, 5] = 2.0 ** 41               # a value outside the domain: the exact route answers
    idx2, ref2 = build(V, O, dim, ids, big)
    for metric in METRICS:
        rank = ranking(ref2, q, metric)
        for t in (float(rank[1][0]), float(rank[1][50]), float(rank[1][n - 1])):
            check(idx2, rank, q, t, metric)
            assert V.last_path() == V.PATH_EXACT_SORT
    qbig = q.copy()
    qbig[3] = 2.0 ** 45                  # a query outside the domain
    for metric in METRICS:
        rank = ranking(ref, qbig, metric)
        check(idx, rank, qbig, float(rank[1][20]), metric)
        assert V.last_path() == V.PATH_EXACT_SORT


def test_nan_status_exactly_when_the_oracle_raises(V, O):
    rng = np.random.default_rng(9)
    n, dim = 1000, 16
    ids = np.arange(n, dtype=np.uint64)
    rows = rng.standard_normal((n, dim))
    rows[500, 3] = np.nan
    idx, ref = build(V, O, dim, ids, rows)
    q = rng.standard_normal(dim)
    for metric in METRICS:
        with pytest.raises(O.OracleError):
            ref.search(q, n, metric)
        with pytest.raises(V.NaNScore):
            idx.search_range_arrays(q, 0.5, metric)
    outside = [int(x) for x in ids if x != 500]
    sub = O.FlatOracle(dim, ids[ids != 500], rows[ids != 500])
    rank = ranking(sub, q, COS)
    check(idx, rank, q, float(rank[1][5]), COS, filt=outside)
    with pytest.raises(V.NaNScore):
        idx.search_range_arrays(q, 0.5, COS, filter=[1, 2, 500, 7])
    lone = O.FlatOracle(dim, ids[500:501], rows[500:501])
    li, ls = lone.search(q, 1, COS)      # a 1-row sort never compares: no error, and NaN >= x is false
    assert np.isnan(ls[0])
    gi, _, total = idx.search_range_arrays(q, -np.inf, COS, filter=[500])
    assert total == 0 and gi.size == 0


# ---- 7. filters ----------------------------------------------------------------------------------
def subsets(rng, ids):
    n = ids.size
    out = [[], [int(ids[rng.integers(n)])]]
    for m in (10, max(1, n // 100), n // 2, n):
        m = min(m, n)
        out.append([int(x) for x in rng.choice(ids, size=m, replace=False)])
    return out


@pytest.mark.parametrize("dim,sizes", [(3, (1, 65, 10_000)), (50, (64, 10_000)), (384, (63, 10_000, 100_000)), (768, (1, 10_000))])
def test_filtered_range_equals_the_oracle_over_the_subset(V, O, dim, sizes):
    rng = np.random.default_rng(100 + dim)
    for n in sizes:
        ids = random_ids(rng, n)
        rows = rng.standard_normal((n, dim))
        idx = V.FlatIndex(dim)
        idx.add_rows(ids, rows, validate=False)
        q = rng.standard_normal(dim)
        for keep in subsets(rng, ids):
            sel = np.isin(ids, np.asarray(sorted(keep), dtype=np.uint64)) if keep else np.zeros(n, bool)
            ref = O.FlatOracle(dim, ids[sel], rows[sel])
            with idx.make_filter(keep) as f:
                for metric in METRICS:
                    if not keep:
                        gi, _, total = idx.search_range_arrays(q, -np.inf, metric, filter=f)
                        assert total == 0 and gi.size == 0
                        continue
                    rank = ranking(ref, q, metric)
                    for t in thresholds(rank[1]):
                        check(idx, rank, q, float(t), metric, filt=f, tag=(dim, n, len(keep)))


def test_filter_follows_adds_and_deletes(V, O):
    rng = np.random.default_rng(11)
    n, dim = 5000, 64
    ids = np.arange(n, dtype=np.uint64) * np.uint64(2)
    rows = rng.standard_normal((n, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    keep = [int(x) for x in ids[1::3]] + [20_001, 20_003]
    q = rng.standard_normal(dim)
    f = idx.make_filter(keep)

    def agree():
        eids, evals = idx.export()
        sel = np.isin(eids, np.asarray(keep, dtype=np.uint64))
        ref = O.FlatOracle(dim, eids[sel], evals[sel])
        for metric in (COS, MAN):
            rank = ranking(ref, q, metric)
            for r in (0, 30, len(ref) - 1):
                check(idx, rank, q, float(rank[1][r]), metric, filt=f)

    agree()
    idx.add(V.Vector(id=20_001, values=list(q * 1.5)))
    agree()
    idx.add_rows(np.array([20_003, 20_007], dtype=np.uint64), rng.standard_normal((2, dim)))
    agree()
    for d in (int(ids[0]), int(ids[4]), 20_003):
        idx.delete(d)
        agree()
    f.close()


# ---- 8. mutations and concurrency ------------------------------------------------------------------
def test_add_delete_range_sequences_against_a_mirrored_oracle(V, O):
    rng = np.random.default_rng(12)
    dim = 50
    idx = V.FlatIndex(dim)
    ref = O.FlatOracle(dim)
    q = rng.standard_normal(dim)
    next_id, live = 1, []
    for step in range(60):
        if live and rng.random() < 0.3:
            d = live.pop(int(rng.integers(len(live))))
            idx.delete(d)
            ref.delete(d)
        else:
            m = int(rng.integers(1, 200))
            new = np.arange(next_id, next_id + m, dtype=np.uint64)
            vals = rng.standard_normal((m, dim))
            idx.add_rows(new, vals)
            ref.extend(new, vals)
            live += new.tolist()
            next_id += m
        if len(ref) == 0:
            continue
        metric = METRICS[step % 4]
        rank = ranking(ref, q, metric)
        for r in (0, len(ref) // 2, len(ref) - 1):
            check(idx, rank, q, float(rank[1][r]), metric)


def test_concurrent_range_and_topk_searches_while_a_writer_adds(V, O):
    rng = np.random.default_rng(13)
    n, dim = 30_000, 128
    ids = np.arange(n, dtype=np.uint64)
    rows = rng.standard_normal((n, dim))
    q = rng.standard_normal(dim)
    extra = [(np.arange(n, n + 500, dtype=np.uint64), np.vstack([q * 2.0, rng.standard_normal((499, dim))])),
             (np.arange(n + 500, n + 900, dtype=np.uint64), np.vstack([q * 3.0, rng.standard_normal((399, dim))]))]
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    ref = O.FlatOracle(dim, ids, rows)
    t = float(ranking(ref, q, COS)[1][49])  # a fixed threshold: 50 rows qualify at first, more after each step
    states = []
    for step in [None] + extra:
        if step is not None:
            ref.extend(*step)
        ri, rs = ranking(ref, q, COS)
        ei, es = expected((ri, rs), t)
        states.append(((ei.tolist(), bits(es)), (ri[:10].tolist(), bits(rs[:10]))))
    answers = [[] for _ in range(8)]
    stop = threading.Event()

    def reader(i):
        while True:
            last = stop.is_set()
            if i % 2 == 0:
                gi, gs, total = idx.search_range_arrays(q, t, COS)
                assert total == gi.size
                answers[i].append((0, (gi.tolist(), bits(gs))))
            else:
                gi, gs = idx.search_arrays(q, 10, COS)
                answers[i].append((1, (gi.tolist(), bits(gs))))
            if last:
                return

    th = [threading.Thread(target=reader, args=(i,)) for i in range(8)]
    for x in th:
        x.start()
    for step in extra:
        idx.add_rows(*step)
    stop.set()
    for x in th:
        x.join()
    for i in range(8):
        assert answers[i]
        for kind, a in answers[i]:
            assert any(a == s[kind] for s in states)
        assert answers[i][-1][1] == states[2][answers[i][-1][0]]  # the pass after the writer finished sees every row


# ---- 9. errors -----------------------------------------------------------------------------------
def test_errors(V):
    rng = np.random.default_rng(14)
    idx = V.FlatIndex(8)
    idx.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    q = np.ones(8)
    with pytest.raises(V.DimensionMismatch):
        idx.search_range_arrays(np.zeros(7), 0.5, COS)
    with pytest.raises(V.IndexOpError, match="metric"):
        idx.search_range_arrays(q, 0.5, 7)
    with pytest.raises(V.IndexOpError, match="NaN"):
        idx.search_range_arrays(q, float("nan"), COS)
    f = idx.make_filter([1, 2])
    tok = f.token
    f.close()
    n_out, tot = C.c_uint64(0), C.c_uint64(0)
    out_i, out_s = np.zeros(4, dtype=np.uint64), np.zeros(4)
    rc = idx._L.vl_index_search_range(idx._h, tok, q.ctypes.data, 8, 0.5, COS, out_i.ctypes.data, out_s.ctypes.data, 4,
                                      C.byref(n_out), C.byref(tot))
    assert rc == 8  # VL_ERR_INVALID_ARG: unknown filter
    with idx.make_filter([1 << 50]) as f:  # an empty filter returns nothing; the dimension check still runs
        assert idx.search_range_arrays(q, -np.inf, COS, filter=f)[2] == 0
        with pytest.raises(V.DimensionMismatch):
            idx.search_range_arrays(np.zeros(7), 0.5, COS, filter=f)
    empty = V.FlatIndex(8)
    assert empty.search_range_arrays(np.zeros(3), 0.5, COS) [2] == 0  # an empty index checks no dimension
    hn = V.HNSWIndex(8)
    hn.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        hn.search_range_arrays(q, 0.5, COS)
    mi = V.MultiFlatIndex(8, [0, 0])
    mi.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        mi.search_range_arrays(q, 0.5, COS)
    res = idx.search_range(q, -np.inf, V.SimilarityMetric.Cosine)
    assert len(res) == 10 and all(isinstance(r, V.SearchResult) for r in res)
