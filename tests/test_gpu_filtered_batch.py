"""Batches of filtered searches with one filter per query (vl_index_search_batch_filters): row i is, ids and f64 score
bits and count, exactly the single filtered search of (query i, filter i) -- FlatIndex::search on the filter's rows in
storage order -- while the jobs share scan launches (vl_index_last_filtered_batch tells how they were routed)."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, EUC, MAN, DOT = 0, 1, 2, 3
METRICS = (COS, EUC, MAN, DOT)
JOBS_VARIANT_BASE = 6_000_000


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
    """n distinct ids below 2^40 in random order (an odd multiplier is a bijection modulo 2^40)."""
    base = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(rng.integers(1 << 20))) % np.uint64(1 << 40)
    return rng.permutation(base)


def near_duplicates(rng, n, dim, count=150):
    """n unit rows; `count` of them differ by far less than the f32 scan resolves, next to the query."""
    rows = rng.standard_normal((n, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    b = rng.choice([-1.0, 1.0], size=dim) / np.sqrt(dim)
    q = b + 0.05 * rng.standard_normal(dim) / np.sqrt(dim)
    d = q - (q @ b) * b
    d /= np.abs(d).max()
    eps = 2.0 ** -12 * 0.5 / np.sqrt(dim) / count
    where = np.sort(rng.choice(np.arange(n), size=count, replace=False))
    rows[where] = b[None, :] + (np.arange(1, count + 1) * eps)[:, None] * d[None, :]
    return rows, q, where


def subset_oracle(O, dim, ids, rows, keep):
    sel = np.isin(ids, np.asarray(sorted(keep), dtype=np.uint64)) if len(keep) else np.zeros(ids.size, bool)
    return O.FlatOracle(dim, ids[sel], rows[sel]), int(sel.sum())


def assert_rows_equal(got, want, what):
    """got = (ids [nq, k], scores, n); want[i] = (ids list, score bits list) of query i."""
    gi, gs, gn = got
    assert len(want) == gi.shape[0]
    for i, (wi, ws) in enumerate(want):
        assert int(gn[i]) == len(wi), (what, i, int(gn[i]), len(wi))
        assert gi[i, : len(wi)].tolist() == wi, (what, i)
        assert bits(gs[i, : len(wi)]) == ws, (what, i)


def mixed_filters(rng, ids, nq, sizes):
    """nq id lists whose sizes cycle through `sizes` (0 = ids the index does not hold)."""
    out = []
    for i in range(nq):
        m = sizes[i % len(sizes)]
        if m == 0:
            out.append([int(x) for x in (np.uint64(1 << 41) + np.arange(5, dtype=np.uint64) + np.uint64(i))])
        else:
            out.append([int(x) for x in rng.choice(ids, size=m, replace=False)])
    return out


class Mix:
    """One index, 37 queries, 37 filters whose sizes cycle through the boundary sizes; the oracle's 200 best per
    (query, filter, metric) computed once -- a smaller k's answer is its prefix (FlatIndex::search sorts, then truncates)."""

    def __init__(self, V, O, dim, sizes=None, n=10_000, nq=37):
        rng = np.random.default_rng(1000 + dim)
        self.n, self.dim, self.nq = n, dim, nq
        self.ids = random_ids(rng, n)
        self.rows = rng.standard_normal((n, dim))
        self.idx = V.FlatIndex(dim)
        self.idx.add_rows(self.ids, self.rows, validate=False)
        self.Q = rng.standard_normal((nq, dim))
        self.keeps = mixed_filters(rng, self.ids, nq, sizes or (0, 1, 3, 63, 64, 65, 1000, n // 2, n))
        self.filters = [self.idx.make_filter(k) for k in self.keeps]
        self.m = [f.rows() for f in self.filters]
        self._O, self._ref = O, {}

    def want(self, metric, k):
        if metric not in self._ref:
            per_query = []
            for i in range(self.nq):
                ref, m = subset_oracle(self._O, self.dim, self.ids, self.rows, self.keeps[i])
                assert m == self.m[i]
                ri, rs = ref.search(self.Q[i], 200, metric) if m else (np.zeros(0, np.uint64), np.zeros(0))
                per_query.append((ri.tolist(), bits(rs)))
            self._ref[metric] = per_query
        return [(ri[:k], rs[:k]) for ri, rs in self._ref[metric]]

    def close(self):
        for f in self.filters:
            f.close()


# ---- 1. oracle parity, one filter per query ---------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 50, 64, 384, 768, 1536])
def test_parity_with_the_oracle_one_filter_per_query(V, O, dim):
    mix = Mix(V, O, dim)
    try:
        for metric in METRICS:
            for k in (1, 10, 60, 61, 200):  # 61 and 200: jobs with min(k, m) <= 60 stay batched, the others go single
                got = mix.idx.search_batch(mix.Q, k, metric, filters=mix.filters)
                assert_rows_equal(got, mix.want(metric, k), (dim, metric, k))
                st = mix.idx.last_filtered_batch()
                assert st["batched"] + st["single"] + st["exact"] == sum(1 for m in mix.m if m > 0)
                if k in (61, 200):
                    assert st["single"] >= sum(1 for m in mix.m if min(k, m) > 60)
                    assert st["batched"] >= 1
    finally:
        mix.close()


# ---- 2. equals the single calls, and takes the route ------------------------------------------------------------
@pytest.mark.parametrize("dim", [50, 384, 1536])
def test_equals_the_single_calls_and_takes_the_batched_route(V, O, dim):
    # sizes at which no job needs more than the 64 lists the finalize kernel takes (1000 rows: 63 workgroups at 4 rows per
    # wave step): nothing forces a second launch, so the whole batch must be ONE launch
    mix = Mix(V, O, dim, sizes=(0, 1, 3, 63, 64, 65, 1000))
    try:
        idx = mix.idx
        for metric, k in ((COS, 10), (EUC, 1), (MAN, 60), (DOT, 61)):
            singles, fast_jobs = [], 0
            for i in range(mix.nq):
                si, ss = idx.search_arrays(mix.Q[i], k, metric, filter=mix.filters[i])
                singles.append((si.tolist(), bits(ss)))
                if mix.m[i] > 0 and V.last_path() == V.PATH_FAST:
                    fast_jobs += 1
            assert fast_jobs >= 2
            got = idx.search_batch(mix.Q, k, metric, filters=mix.filters)
            st = idx.last_filtered_batch()
            assert_rows_equal(got, singles, (dim, metric, k))
            # the expectation comes from the single path: every job it answers on the fast path is batched
            assert st["batched"] == fast_jobs, (st, fast_jobs)
            assert st["launches"] == 1, st
        # one shared filter through the old entry point: the n_filters == 1 case of the same path
        f = mix.filters[6]  # 1000 rows
        singles, fast_jobs = [], 0
        for i in range(mix.nq):
            si, ss = idx.search_arrays(mix.Q[i], 10, COS, filter=f)
            singles.append((si.tolist(), bits(ss)))
            fast_jobs += 1 if V.last_path() == V.PATH_FAST else 0
        got = idx.search_batch(mix.Q, 10, COS, filter=f)
        st = idx.last_filtered_batch()
        assert_rows_equal(got, singles, (dim, "shared"))
        assert st["batched"] == fast_jobs and st["launches"] == 1, (st, fast_jobs)
    finally:
        mix.close()


# ---- 3. pass accounting -----------------------------------------------------------------------------------------
def test_one_pass_per_launch_and_only_the_subset_rows(V):
    rng = np.random.default_rng(3)
    n, dim, nf, m = 20_000, 384, 40, 200
    ids = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    rows = rng.standard_normal((n, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    filters = [idx.make_filter(rng.choice(ids, size=m, replace=False)) for _ in range(nf)]
    try:
        Q = rng.standard_normal((nf, dim))
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
        for metric in (COS, DOT):
            idx.search_batch(Q, 10, metric, filters=filters)  # warm
            idx.profile_read()
            idx.profile_enable(True)
            idx.search_batch(Q, 10, metric, filters=filters)
            idx.profile_enable(False)
            passes, _, nbytes = idx.profile_read()
            st = idx.last_filtered_batch()
            assert st == {"batched": nf, "single": 0, "exact": 0, "launches": 1}, st
            assert passes == 1 and nbytes <= 1.05 * nf * m * (dim * 4 + 8), (passes, nbytes)
            assert JOBS_VARIANT_BASE <= idx.last_scan()["variant"] < JOBS_VARIANT_BASE + 1_000_000
        # 513 jobs: two launches, two passes
        many = [filters[i % nf] for i in range(513)]
        Qm = np.ascontiguousarray(Q[np.arange(513) % nf])
        idx.profile_read()
        idx.profile_enable(True)
        bi, bs, bn = idx.search_batch(Qm, 10, COS, filters=many)
        idx.profile_enable(False)
        passes, _, _ = idx.profile_read()
        st = idx.last_filtered_batch()
        assert st["launches"] == 2 and passes == 2 and st["batched"] == 513, (st, passes)
        first = idx.search_batch(Q, 10, COS, filters=filters)
        for i in range(513):
            assert bi[i].tolist() == first[0][i % nf].tolist() and bits(bs[i]) == bits(first[1][i % nf])
    finally:
        for f in filters:
            f.close()


# ---- 4. ties ----------------------------------------------------------------------------------------------------
def test_ties_resolve_by_position_in_every_job(V, O):
    rng = np.random.default_rng(9)
    n, dim = 5000, 384
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    q = rng.standard_normal(dim)
    planted = [10, 400, 401, 2500, 4999]  # equal best rows, inside several overlapping filters and outside them
    rows[planted] = q * 3.0
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    keeps = [[int(ids[p]) for p in (400, 2500, 4999)] + [int(x) for x in ids[::5]],
             [int(ids[p]) for p in (401, 2500)] + [int(x) for x in ids[1::3]],
             [int(ids[p]) for p in (10, 400, 401, 2500, 4999)],
             [int(x) for x in ids[2::7]],
             [int(ids[4999])] + [int(x) for x in ids[:2000]]]
    refs = [subset_oracle(O, dim, ids, rows, kp)[0] for kp in keeps]
    Q = np.tile(q, (len(keeps), 1))
    for metric in METRICS:
        for k in (1, 3, 10):
            got = idx.search_batch(Q, k, metric, filters=keeps)  # one-shot filters from id lists
            want = []
            for ref in refs:
                ri, rs = ref.search(q, k, metric)
                want.append((ri.tolist(), bits(rs)))
            assert_rows_equal(got, want, (metric, k))


# ---- 5. uncertified jobs inside a batch -------------------------------------------------------------------------
def test_uncertified_jobs_are_redone_exactly_beside_batched_ones(V, O):
    rng = np.random.default_rng(3)
    n, dim, k = 40_000, 384, 10
    rows, q, where = near_duplicates(rng, n, dim)
    ids = np.arange(n, dtype=np.uint64) + np.uint64(100)
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    near = [int(ids[p]) for p in where]
    far_pool = np.setdiff1d(ids, np.asarray(near, dtype=np.uint64))
    keeps = []
    for j in range(8):
        some = [int(x) for x in rng.choice(far_pool, size=3000, replace=False)]
        keeps.append(near + some if j % 2 == 0 else some)
    filters = [idx.make_filter(kp) for kp in keeps]
    try:
        Q = np.tile(q, (len(keeps), 1))
        for metric in (COS, EUC, DOT):
            want = []
            for kp in keeps:
                ri, rs = subset_oracle(O, dim, ids, rows, kp)[0].search(q, k, metric)
                want.append((ri.tolist(), bits(rs)))
            got = idx.search_batch(Q, k, metric, filters=filters)
            st = idx.last_filtered_batch()
            assert_rows_equal(got, want, metric)
            # The 150 near rows' scores are 1.4e-8 apart: ranks 10 and 64 differ by under 1e-6, far inside the cosine and
            # dot bounds' 2 (n + 4) u = 4.6e-5, so no list holding them can be certified.  (The Euclidean bound is relative
            # to the distance, 0.05 here: 2.3e-6 against 1.5e-5 between those ranks -- it does certify, rightly.)
            if metric in (COS, DOT):
                assert st["exact"] >= 1 and st["batched"] >= 1, (metric, st)
            assert st["batched"] + st["exact"] + st["single"] == len(keeps), st
            for path in (V.PATH_EXACT_SELECT, V.PATH_EXACT_SORT):
                idx.force_path(path)
                try:
                    got = idx.search_batch(Q, k, metric, filters=filters)
                    assert V.last_path() == path
                    st = idx.last_filtered_batch()
                finally:
                    idx.force_path(0)
                assert_rows_equal(got, want, (metric, path))
                assert st == {"batched": 0, "single": len(keeps), "exact": 0, "launches": 0}, st
    finally:
        for f in filters:
            f.close()


# ---- 6. mutations -----------------------------------------------------------------------------------------------
def test_filters_follow_adds_and_deletes_through_batch_calls(V, O):
    rng = np.random.default_rng(6)
    n, dim = 5000, 64
    ids = np.arange(n, dtype=np.uint64) * np.uint64(2)
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rng.standard_normal((n, dim)), validate=False)
    late = [20_001, 20_003, 20_005]  # ids that arrive later
    keeps = [[int(x) for x in ids[1::3]] + late, [int(x) for x in ids[:40]] + late[:1], [int(x) for x in ids[::2]],
             late, [int(x) for x in ids[4::5]] + late[1:]]
    filters = [idx.make_filter(kp) for kp in keeps]
    Q = rng.standard_normal((len(keeps), dim))

    def agree():
        eids, evals = idx.export()
        for metric in (COS, MAN):
            got = idx.search_batch(Q, 10, metric, filters=filters)  # resolves whatever is stale, once each
            want = []
            for i, kp in enumerate(keeps):
                ref, m = subset_oracle(O, dim, eids, evals, kp)
                ri, rs = ref.search(Q[i], 10, metric) if m else (np.zeros(0, np.uint64), np.zeros(0))
                want.append((ri.tolist(), bits(rs)))
            assert_rows_equal(got, want, metric)
        for f, kp in zip(filters, keeps):
            assert f.rows() == int(np.isin(eids, np.asarray(kp, dtype=np.uint64)).sum())

    try:
        agree()
        idx.add(V.Vector(id=20_001, values=list(rng.standard_normal(dim))))
        agree()
        idx.add_rows(np.array([20_003, 20_005, 20_007], dtype=np.uint64), rng.standard_normal((3, dim)))
        agree()
        for d in (int(ids[0]), int(ids[4]), int(ids[1]), 20_003):  # deletes in front of allowed rows shift their positions
            idx.delete(d)
            agree()
    finally:
        for f in filters:
            f.close()


# ---- 7. errors and edges ----------------------------------------------------------------------------------------
def raw_batch(idx, toks, Q, k, metric, stride, q_len=None):
    """vl_index_search_batch_filters as it is: (rc, ids [nq, stride], scores, n)."""
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    nq = Q.shape[0]
    toks = np.ascontiguousarray(toks, dtype=np.uint64)
    ids = np.zeros((max(nq, 1), max(stride, 1)), dtype=np.uint64)
    scores = np.zeros((max(nq, 1), max(stride, 1)))
    n = np.full(max(nq, 1), 77, dtype=np.uint64)
    rc = idx._L.vl_index_search_batch_filters(idx._h, toks.ctypes.data_as(C.POINTER(C.c_uint64)), toks.size,
                                              Q.ctypes.data_as(C.POINTER(C.c_double)), nq, Q.shape[1] if q_len is None else q_len,
                                              k, metric, stride, ids.ctypes.data_as(C.POINTER(C.c_uint64)),
                                              scores.ctypes.data_as(C.POINTER(C.c_double)), n.ctypes.data_as(C.POINTER(C.c_uint64)))
    return rc, ids, scores, n


def test_errors_and_edges(V):
    rng = np.random.default_rng(8)
    n, dim, nq = 1000, 16, 9
    ids = np.arange(n, dtype=np.uint64)
    rows = rng.standard_normal((n, dim))
    rows[500, 3] = np.nan
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    Q = rng.standard_normal((nq, dim))
    clean = [[int(x) for x in rng.choice(np.delete(ids, 500), size=50, replace=False)] for _ in range(nq)]
    filters = [idx.make_filter(kp) for kp in clean]
    bad = idx.make_filter(clean[5] + [500])
    try:
        # a NaN row outside every subset: all answers right
        got = idx.search_batch(Q, 10, COS, filters=filters)
        for i in range(nq):
            si, ss = idx.search_arrays(Q[i], 10, COS, filter=filters[i])
            assert got[0][i].tolist() == si.tolist() and bits(got[1][i]) == bits(ss) and int(got[2][i]) == 10
        # a NaN row inside job 5's subset
        with_bad = filters[:5] + [bad] + filters[6:]
        with pytest.raises(V.NaNScore):
            idx.search_batch(Q, 10, COS, filters=with_bad)
        rc, ri, rs, rn = raw_batch(idx, [f.token for f in with_bad], Q, 10, COS, 10)
        assert rc != 0 and rn.tolist() == [10] * 5 + [0] * 4
        for i in range(5):
            assert ri[i].tolist() == got[0][i].tolist() and bits(rs[i]) == bits(got[1][i])
        toks = [f.token for f in filters]
        # n_filters is 1 or nq
        rc, _, _, rn = raw_batch(idx, toks[:4], Q, 10, COS, 10)
        assert rc == 8 and rn.tolist() == [0] * nq and "filter" in V._last_error()
        # a token that is 0 or unknown, anywhere in the array: the single call's status, before the metric is looked at
        for bad_tok in (0, 1 << 62):
            rc, _, _, rn = raw_batch(idx, toks[:7] + [bad_tok] + toks[8:], Q, 10, 7, 10)
            assert rc == 8 and "unknown or destroyed filter" in V._last_error() and rn.tolist() == [0] * nq
        rc, _, _, _ = raw_batch(idx, toks, Q, 10, 7, 10)  # then the metric
        assert rc == 8 and "metric" in V._last_error()
        # the dimension check runs whenever the index is not empty, even if every subset is empty
        with idx.make_filter([1 << 50]) as empty:
            with pytest.raises(V.DimensionMismatch):
                idx.search_batch(np.zeros((3, dim - 1)), 3, COS, filters=[empty] * 3)
            got0 = idx.search_batch(np.zeros((3, dim)), 3, COS, filters=[empty] * 3)
            assert got0[2].tolist() == [0, 0, 0]
        # k == 0 and nq == 0: OK, nothing written
        rc, _, _, rn = raw_batch(idx, toks, Q, 0, COS, 10)
        assert rc == 0 and rn.tolist() == [0] * nq
        rc, _, _, rn = raw_batch(idx, [], np.zeros((0, dim)), 10, COS, 10)
        assert rc == 0 and rn.tolist() == [77]
        # capped at out_stride
        rc, ri, _, rn = raw_batch(idx, toks, Q, 10, COS, 4)
        assert rc == 0 and rn.tolist() == [4] * nq and ri[:, :4].tolist() == got[0][:, :4].tolist()
        # a closed filter in the middle of the list
        closed = idx.make_filter(clean[0])
        closed.close()
        with pytest.raises(V.IndexOpError, match="unknown or destroyed filter"):
            idx.search_batch(Q, 10, COS, filters=filters[:4] + [closed] + filters[5:])
        # a filter of another index; filter= and filters= together; a wrong length
        other = V.FlatIndex(dim)
        other.add_rows(ids[:10], rng.standard_normal((10, dim)))
        with other.make_filter([1, 2]) as of:
            with pytest.raises(ValueError):
                idx.search_batch(Q, 10, COS, filters=filters[:8] + [of])
        with pytest.raises(ValueError):
            idx.search_batch(Q, 10, COS, filter=filters[0], filters=filters)
        with pytest.raises(ValueError):
            idx.search_batch(Q, 10, COS, filters=filters[:3])
        # HNSW and multi-GPU handles refuse
        hn = V.HNSWIndex(dim)
        hn.add_rows(ids[:10], rng.standard_normal((10, dim)))
        mi = V.MultiFlatIndex(dim, [0, 0])
        mi.add_rows(ids[:10], rng.standard_normal((10, dim)))
        for h in (hn, mi):
            rc, _, _, _ = raw_batch(h, toks, Q, 10, COS, 10)
            assert rc == 8 and "single-GPU flat" in V._last_error()
            a = C.c_uint64(0)
            assert h._L.vl_index_last_filtered_batch(h._h, C.byref(a), None, None, None) == 8
    finally:
        bad.close()
        for f in filters:
            f.close()


# ---- 8. concurrency ---------------------------------------------------------------------------------------------
def test_concurrent_batches_over_overlapping_filters(V):
    rng = np.random.default_rng(12)
    n, dim, nt, nq = 20_000, 128, 8, 12
    ids = np.arange(n, dtype=np.uint64)
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rng.standard_normal((n, dim)), validate=False)
    keeps = [[int(x) for x in ids[j::3 + j]] for j in range(6)]  # overlapping
    filters = [idx.make_filter(kp) for kp in keeps]
    Qs = [rng.standard_normal((nq, dim)) for _ in range(nt)]
    picks = [[filters[(t + i) % len(filters)] for i in range(nq)] for t in range(nt)]
    try:
        idx.delete(3)  # every filter is stale when the threads start
        idx.add(V.Vector(id=n + 1, values=list(rng.standard_normal(dim))))
        clone = idx.clone()
        lone = []
        cfilters = [clone.make_filter(kp) for kp in keeps]
        for t in range(nt):
            lone.append(clone.search_batch(Qs[t], 10, COS, filters=[cfilters[(t + i) % len(filters)] for i in range(nq)]))
        for f in cfilters:
            f.close()
        out, errs = [None] * nt, []

        def run(t):
            try:
                out[t] = idx.search_batch(Qs[t], 10, COS, filters=picks[t])
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=run, args=(t,)) for t in range(nt)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for t in range(nt):
            assert out[t][0].tolist() == lone[t][0].tolist() and bits(out[t][1]) == bits(lone[t][1])
            assert out[t][2].tolist() == lone[t][2].tolist()
    finally:
        for f in filters:
            f.close()


# ---- 9. big jobs keep the machine -------------------------------------------------------------------------------
def test_whole_index_filters_among_small_ones(V):
    # The plan's P4 (no launch leaves the machine idle because of a cap) is checked on this very mix by the CPU test of
    # subset_batch_plan.hpp.  The resident workgroup count the library planned with is not part of the public interface,
    # so P4 is not recomputed here: this asserts the answers and that both kinds of job were served.
    rng = np.random.default_rng(21)
    n, dim = 200_000, 64
    ids = np.arange(n, dtype=np.uint64)
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rng.standard_normal((n, dim)), validate=False)
    whole = idx.make_filter(ids)
    small = [idx.make_filter(rng.choice(ids, size=50, replace=False)) for _ in range(20)]
    try:
        filters = list(small)
        for at in (0, 11, 22):
            filters.insert(at, whole)
        Q = rng.standard_normal((len(filters), dim))
        got = idx.search_batch(Q, 10, COS, filters=filters)
        st = idx.last_filtered_batch()
        for i, f in enumerate(filters):
            si, ss = idx.search_arrays(Q[i], 10, COS, filter=f)
            assert got[0][i].tolist() == si.tolist() and bits(got[1][i]) == bits(ss) and int(got[2][i]) == 10
        assert st["batched"] + st["single"] + st["exact"] == len(filters), st
        assert st["batched"] >= 20 and st["launches"] >= 1, st
    finally:
        whole.close()
        for f in small:
            f.close()


# ---- 10. client mirror ------------------------------------------------------------------------------------------
def test_client_search_texts_with_a_predicate_per_query(V):
    from vectorlite_amd import client

    class Embedder:
        def generate_embedding(self, text):
            return list(np.random.default_rng(sum(text.encode()) * 7919 % (1 << 32)).standard_normal(16))

        def dimension(self):
            return 16

    cl = client.VectorLiteClient(Embedder())
    cl.create_collection("docs", client.IndexType.Flat)
    for i in range(300):
        cl.add_text_to_collection("docs", f"text {i}", {"user": i % 7})
    wheres = [lambda md: md["user"] == 3, None, lambda md: md["user"] in (1, 2), lambda md: md["user"] == 3,  # noqa: E731
              lambda md: md["user"] > 100]
    texts = [f"query {i}" for i in range(len(wheres))]
    res = cl.search_texts_in_collection("docs", texts, 5, V.SimilarityMetric.Cosine, wheres=wheres)
    assert len(res) == len(texts)
    for text, where, got in zip(texts, wheres, res):
        one = cl.search_text_in_collection("docs", text, 5, V.SimilarityMetric.Cosine, where=where)
        assert [(r.id, r.text, r.metadata) for r in got] == [(r.id, r.text, r.metadata) for r in one]
        assert bits([r.score for r in got]) == bits([r.score for r in one])
    assert res[4] == [] and len(res[0]) == 5 and len(res[1]) == 5
    plain = cl.search_texts_in_collection("docs", texts[:2], 5)  # no predicates at all: the default metric, search_batch
    assert [[r.id for r in row] for row in plain] == [[r.id for r in cl.search_text_in_collection("docs", t, 5)] for t in texts[:2]]
