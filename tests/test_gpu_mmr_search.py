"""Diversified (MMR) search (vl_index_search_mmr) against the oracle.  The expected answer is the contract's pseudocode
restated in Python below: candidates from oracle.FlatOracle.search, every pairwise similarity from oracle.calculate,
v in plain Python floats.  Ids and score bits are compared with == for every query."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, EUC, MAN, DOT = 0, 1, 2, 3
METRICS = (COS, EUC, MAN, DOT)
K_FETCH = ((1, 1), (4, 20), (10, 60), (10, 61), (50, 300), (64, 1024))
LAMBDAS = (0.0, 0.25, 0.5, 1.0)


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


def clustered(rng, n, dim, unit=True):
    """a few hundred centres plus small noise: the best candidates of a query are near-copies of each other"""
    centres = rng.standard_normal((min(300, max(1, n // 16)), dim))
    rows = centres[rng.integers(centres.shape[0], size=n)] + 0.05 * rng.standard_normal((n, dim))
    if unit:
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    return np.ascontiguousarray(rows)


def mmr_reference(O, metric, rel, cand_rows, k, lam, cache):
    """The contract's selection, operation for operation.  rel / cand_rows: the candidates in the search's ranking.
    cache: (i, j) -> calculate(metric, row[i], row[j]) for one candidate list (shared by its prefixes)."""
    n = len(rel)
    if n == 0 or k == 0:
        return []
    one_minus = 1.0 - lam
    sel, chosen, red = [0], [False] * n, [-math.inf] * n
    chosen[0] = True
    while len(sel) < min(k, n):
        j = sel[-1]
        for i in range(n):
            if chosen[i]:
                continue
            s = cache.get((i, j))
            if s is None:
                s = cache[(i, j)] = O.calculate(metric, cand_rows[i], cand_rows[j])
            if s > red[i]:
                red[i] = s
        best, v_best = None, None
        for i in range(n):
            if chosen[i]:
                continue
            v = (lam * rel[i]) - (one_minus * red[i])
            if best is None or v > v_best:
                best, v_best = i, v
        sel.append(best)
        chosen[best] = True
    return sel


class Case:
    """An index, its rows and the oracle of the same rows whose ids are the storage positions (candidates are rows)."""

    def __init__(self, V, O, dim, ids, rows):
        self.V, self.O, self.dim = V, O, dim
        self.ids = np.ascontiguousarray(ids, dtype=np.uint64)
        self.rows = np.ascontiguousarray(rows, dtype=np.float64)
        self.idx = V.FlatIndex(dim)
        self.idx.add_rows(self.ids, self.rows, validate=False)
        self.ref = O.FlatOracle(dim, np.arange(self.ids.size, dtype=np.uint64), self.rows)
        self._cand = {}

    def candidates(self, q, fetch_k, metric, positions=None):
        """(positions, rel, sims cache) of search(q, fetch_k): over the subset `positions` (ascending) when given"""
        key = (q.tobytes(), metric, None if positions is None else positions.tobytes())
        hit = self._cand.get(key)
        if hit is None or hit[0].size < min(fetch_k, hit[3]):
            if positions is None:
                ref, total = self.ref, self.ids.size
            else:  # the FlatIndex of the subset's rows in their storage order
                ref, total = self.O.FlatOracle(self.dim, positions, self.rows[positions]), positions.size
            want = min(max(fetch_k, 1024), total)
            p, s = ref.search(q, want, metric) if total else (np.zeros(0, np.uint64), np.zeros(0))
            hit = (p, s, {}, total)
            self._cand[key] = hit
        p, s, cache, total = hit
        m = min(fetch_k, total)
        return p[:m], s[:m], cache  # search(q, fetch_k) is the prefix of search(q, more)

    def expect(self, q, k, fetch_k, lam, metric, positions=None):
        p, s, cache = self.candidates(q, fetch_k, metric, positions)
        sel = mmr_reference(self.O, metric, s.tolist(), self.rows[p.astype(np.int64)], k, lam, cache)
        return self.ids[p[sel].astype(np.int64)], s[sel], sel

    def check(self, q, k, fetch_k, lam, metric, filt=None, positions=None, tag=None):
        ei, es, sel = self.expect(q, k, fetch_k, lam, metric, positions)
        gi, gs = self.idx.search_mmr_arrays(q, k, fetch_k, lam, metric, filter=filt)
        assert gi.tolist() == ei.tolist(), (tag, metric, k, fetch_k, lam)
        assert bits(gs) == bits(es), (tag, metric, k, fetch_k, lam)
        return sel


# ---- 1. parity -----------------------------------------------------------------------------------
# dim 3 and 50: generic scan strides; 384: the headline stride; 800: the f64 query form (above 768 kernel-argument floats)
@pytest.mark.parametrize("dim", [3, 50, 384, 800])
@pytest.mark.parametrize("n", [1, 5, 5000, 200_000])
def test_parity_with_the_restated_selection(V, O, dim, n):
    rng = np.random.default_rng(1000 * dim + n % 977)
    case = Case(V, O, dim, random_ids(rng, n), clustered(rng, n, dim))
    reordered, paths = 0, set()
    for metric in METRICS:
        q = case.rows[rng.integers(n)] + 0.02 * rng.standard_normal(dim)  # a question about one of the paragraphs
        for k, fetch_k in K_FETCH:
            for lam in LAMBDAS:
                sel = case.check(q, k, fetch_k, lam, metric, tag=(dim, n))
                if lam == 0.5 and sel != list(range(len(sel))):
                    reordered += 1
            paths.add((fetch_k <= 60, V.last_path()))
    if n >= 5000:
        # otherwise the comparison proves nothing: redundancy must actually reorder the answer
        assert reordered > 0, (dim, n)
        # the certified fast path and the exact routes both fed the selection
        assert (True, V.PATH_FAST) in paths and paths & {(False, V.PATH_EXACT_SELECT), (False, V.PATH_EXACT_SORT)}, paths


def test_lambda_one_is_the_plain_top_k_and_smaller_k_is_a_prefix(V, O):
    rng = np.random.default_rng(21)
    n, dim = 20_000, 128
    case = Case(V, O, dim, random_ids(rng, n), clustered(rng, n, dim))
    for metric in METRICS:
        for _ in range(3):
            q = case.rows[rng.integers(n)] + 0.02 * rng.standard_normal(dim)
            for k, fetch_k in ((4, 20), (10, 60), (10, 61), (50, 300)):
                gi, gs = case.idx.search_mmr_arrays(q, k, fetch_k, 1.0, metric)
                si, ss = case.idx.search_arrays(q, fetch_k, metric)
                assert gi.tolist() == si[:k].tolist() and bits(gs) == bits(ss[:k])
            for lam in (0.0, 0.5):
                for fetch_k in (20, 100):
                    i10, s10 = case.idx.search_mmr_arrays(q, 10, fetch_k, lam, metric)
                    i3, s3 = case.idx.search_mmr_arrays(q, 3, fetch_k, lam, metric)
                    assert i3.tolist() == i10[:3].tolist() and bits(s3) == bits(s10[:3])
                    case.check(q, 10, fetch_k, lam, metric)


# ---- 2. ties -------------------------------------------------------------------------------------
def test_duplicated_rows_and_grid_values_resolve_ties_by_rank(V, O):
    rng = np.random.default_rng(22)
    n, dim = 4000, 48
    rows = clustered(rng, n, dim, unit=False)
    ids = random_ids(rng, n)
    # exact copies under different ids: adjacent in storage, and far apart
    for src in (100, 101, 102, 1500):
        rows[src + 1] = rows[src]
        rows[(src * 7 + 2000) % n] = rows[src]
    rows[3000:3040] = rows[100]
    case = Case(V, O, dim, ids, rows)
    for metric in METRICS:
        for q in (rows[100] + 0.01 * rng.standard_normal(dim), rows[1500].copy(), rows[100].copy()):
            for k, fetch_k in ((10, 20), (30, 60), (40, 100), (64, 1024)):
                for lam in LAMBDAS:
                    case.check(q, k, fetch_k, lam, metric, tag="copies")
    grid = rng.integers(-2, 3, size=(n, 6)).astype(np.float64)  # 5^6 cells for 4000 rows: equal scores, equal v
    gcase = Case(V, O, 6, ids, grid)
    for metric in METRICS:
        for q in (grid[7].copy(), np.array([1.0, 0, -1, 2, 0, 1]), np.zeros(6)):
            for k, fetch_k in ((10, 20), (40, 60), (40, 200)):
                for lam in LAMBDAS:
                    gcase.check(q, k, fetch_k, lam, metric, tag="grid")


# ---- 3. filters ----------------------------------------------------------------------------------
def test_filtered_candidates_are_the_subset_search(V, O):
    rng = np.random.default_rng(23)
    n, dim = 20_000, 64
    case = Case(V, O, dim, random_ids(rng, n), clustered(rng, n, dim))
    subsets = [np.zeros(0, np.int64), np.array([777]), np.sort(rng.choice(n, n // 100, replace=False)),
               np.sort(rng.choice(n, n // 2, replace=False))]
    q = case.rows[4242] + 0.02 * rng.standard_normal(dim)
    for pos in subsets:
        id_list = [int(x) for x in case.ids[pos]]
        with case.idx.make_filter(id_list) as f:
            for metric in METRICS:
                for k, fetch_k in ((4, 20), (10, 60), (50, 300), (64, 1024)):  # 300 and 1024 exceed the 1 % subset
                    for lam in (0.0, 0.5, 1.0):
                        case.check(q, k, fetch_k, lam, metric, filt=f, positions=pos.astype(np.uint64), tag=("token", pos.size))
                case.check(q, 10, 60, 0.5, metric, filt=id_list, positions=pos.astype(np.uint64), tag=("list", pos.size))
    with case.idx.make_filter([1 << 50]) as f:  # an empty subset: nothing, but the dimension check still runs
        gi, gs = case.idx.search_mmr_arrays(q, 4, 20, 0.5, COS, filter=f)
        assert gi.size == 0 and gs.size == 0
        with pytest.raises(V.DimensionMismatch):
            case.idx.search_mmr_arrays(np.zeros(dim - 1), 4, 20, 0.5, COS, filter=f)


def test_a_filter_gone_stale_is_resolved_again(V, O):
    rng = np.random.default_rng(24)
    n, dim = 3000, 32
    ids = np.arange(n, dtype=np.uint64) * 3
    rows = clustered(rng, n, dim)
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    wanted = [int(x) for x in ids[::2]] + [9001, 9004]
    f = idx.make_filter(wanted)
    # rows leave and arrive between the filter's creation and its use
    for gone in (0, 6, 600):
        idx.delete(gone)
    extra = clustered(rng, 4, dim)
    idx.add_rows(np.array([9001, 9002, 9003, 9004], dtype=np.uint64), extra, validate=False)
    keep = ~np.isin(ids, [0, 6, 600])
    now_ids = np.concatenate([ids[keep], np.array([9001, 9002, 9003, 9004], dtype=np.uint64)])
    now_rows = np.concatenate([rows[keep], extra])
    mirror = Case.__new__(Case)
    mirror.V, mirror.O, mirror.dim, mirror.ids, mirror.rows, mirror.idx, mirror._cand = V, O, dim, now_ids, now_rows, idx, {}
    mirror.ref = O.FlatOracle(dim, np.arange(now_ids.size, dtype=np.uint64), now_rows)
    pos = np.nonzero(np.isin(now_ids, wanted))[0].astype(np.uint64)
    q = rows[1000] + 0.02 * rng.standard_normal(dim)
    for metric in METRICS:
        for lam in (0.25, 0.5):
            mirror.check(q, 10, 60, lam, metric, filt=f, positions=pos)
            mirror.check(q, 10, 60, lam, metric)
    f.close()


# ---- 4. routes -----------------------------------------------------------------------------------
def test_forced_exact_paths_give_the_same_answers(V, O):
    rng = np.random.default_rng(25)
    n, dim = 30_000, 96
    case = Case(V, O, dim, random_ids(rng, n), clustered(rng, n, dim))
    sub = np.sort(rng.choice(n, 3000, replace=False))
    q = case.rows[99] + 0.02 * rng.standard_normal(dim)
    with case.idx.make_filter([int(x) for x in case.ids[sub]]) as f:
        for path in (0, V.PATH_EXACT_SELECT, V.PATH_EXACT_SORT):
            case.idx.force_path(path)
            try:
                for metric in METRICS:
                    for k, fetch_k in ((4, 20), (10, 61), (50, 300)):
                        case.check(q, k, fetch_k, 0.5, metric, tag=("path", path))
                        if path == V.PATH_EXACT_SORT:
                            assert V.last_path() == path
                        elif path:  # the selection rounds serve as many ranks as the index size allows, the sort the rest
                            assert V.last_path() in (V.PATH_EXACT_SELECT, V.PATH_EXACT_SORT)
                        case.check(q, k, fetch_k, 0.5, metric, filt=f, positions=sub.astype(np.uint64), tag=("path", path, "f"))
            finally:
                case.idx.force_path(0)


def test_rows_outside_the_fast_path_domain(V, O):
    rng = np.random.default_rng(26)
    n, dim = 5000, 64
    rows = clustered(rng, n, dim, unit=False)
    rows[99, 5] = 2.0 ** 41  # a value outside the domain: the exact route finds the candidates
    rows[17] = 0.0           # a zero row: cosine 0.0 with everything
    case = Case(V, O, dim, random_ids(rng, n), rows)
    qs = [rows[200] + 0.02 * rng.standard_normal(dim), rows[99].copy(), np.zeros(dim)]
    for metric in METRICS:
        for q in qs:
            for k, fetch_k in ((4, 20), (10, 60), (50, 300)):
                for lam in (0.0, 0.5, 1.0):
                    case.check(q, k, fetch_k, lam, metric, tag="domain")
                assert V.last_path() in (V.PATH_EXACT_SELECT, V.PATH_EXACT_SORT)
    qbig = qs[0].copy()
    qbig[3] = 2.0 ** 45      # a query outside the domain, on in-domain rows
    clean = Case(V, O, dim, case.ids, clustered(rng, n, dim))
    for metric in METRICS:
        clean.check(qbig, 10, 60, 0.5, metric, tag="qbig")
        assert V.last_path() in (V.PATH_EXACT_SELECT, V.PATH_EXACT_SORT)


def test_nan_status_exactly_when_the_search_returns_it(V, O):
    rng = np.random.default_rng(9)
    n, dim = 1000, 16
    ids = np.arange(n, dtype=np.uint64)
    rows = rng.standard_normal((n, dim))
    rows[500, 3] = np.nan
    case = Case(V, O, dim, ids, rows)
    q = rng.standard_normal(dim)
    for metric in METRICS:
        with pytest.raises(O.OracleError):
            case.ref.search(q, 20, metric)
        with pytest.raises(V.NaNScore):
            case.idx.search_arrays(q, 20, metric)
        for k, fetch_k in ((1, 1), (4, 20), (10, 61), (50, 300)):
            with pytest.raises(V.NaNScore):
                case.idx.search_mmr_arrays(q, k, fetch_k, 0.5, metric)
    outside = np.array([p for p in range(n) if p != 500], dtype=np.uint64)
    for k, fetch_k in ((4, 20), (50, 300)):
        case.check(q, k, fetch_k, 0.5, COS, filt=[int(x) for x in outside], positions=outside)
    with pytest.raises(V.NaNScore):
        case.idx.search_mmr_arrays(q, 2, 4, 0.5, COS, filter=[1, 2, 500, 7])
    gi, gs = case.idx.search_mmr_arrays(q, 2, 4, 0.5, COS, filter=[500])  # a 1-row sort never compares
    assert gi.tolist() == [500] and np.isnan(gs[0])
    nq = q.copy()
    nq[0] = np.nan
    clean = Case(V, O, dim, ids, rng.standard_normal((n, dim)))
    with pytest.raises(V.NaNScore):
        clean.idx.search_arrays(nq, 20, DOT)
    with pytest.raises(V.NaNScore):
        clean.idx.search_mmr_arrays(nq, 4, 20, 0.5, DOT)


# ---- 5. the C entry point ------------------------------------------------------------------------
def raw_call(idx, q, k, fetch_k, lam, metric, cap, token=0, slots=80):
    guard_i, guard_s = np.uint64(0xDEADBEEFDEADBEEF), -12345.678
    out_i = np.full(slots, guard_i, dtype=np.uint64)
    out_s = np.full(slots, guard_s)
    n_out = C.c_uint64(99)
    rc = idx._L.vl_index_search_mmr(idx._h, token, q.ctypes.data, q.size, k, fetch_k, lam, metric, cap, out_i.ctypes.data,
                                    out_s.ctypes.data, C.byref(n_out))
    m = int(n_out.value)
    assert (out_i[m:] == guard_i).all() and (out_s[m:] == guard_s).all()  # nothing beyond what was announced
    return rc, out_i[:m].copy(), out_s[:m].copy()


def test_capacity_writes_the_prefix_and_nothing_beyond(V, O):
    rng = np.random.default_rng(27)
    n, dim = 8000, 40
    case = Case(V, O, dim, random_ids(rng, n), clustered(rng, n, dim))
    q = case.rows[5] + 0.02 * rng.standard_normal(dim)
    for metric in (COS, EUC):
        for k, fetch_k in ((10, 60), (50, 300)):
            ei, es, _ = case.expect(q, k, fetch_k, 0.5, metric)
            for cap in (0, 1, 3, k - 1, k, k + 5):
                rc, gi, gs = raw_call(case.idx, q, k, fetch_k, 0.5, metric, cap)
                want = min(k, cap)
                assert rc == 0 and gi.size == want
                assert gi.tolist() == ei[:want].tolist() and bits(gs) == bits(es[:want])
    rc, gi, _ = raw_call(case.idx, q, 0, 0, 0.5, COS, 8)  # k = 0
    assert rc == 0 and gi.size == 0
    few = Case(V, O, dim, case.ids[:7], case.rows[:7])    # fewer rows than k: min(k, n) entries
    ei, es, _ = few.expect(q, 10, 60, 0.5, COS)
    rc, gi, gs = raw_call(few.idx, q, 10, 60, 0.5, COS, 64)
    assert rc == 0 and gi.size == 7 and gi.tolist() == ei.tolist() and bits(gs) == bits(es)


def test_errors_and_refusals(V):
    rng = np.random.default_rng(14)
    idx = V.FlatIndex(8)
    idx.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    q = np.ones(8)
    with pytest.raises(V.DimensionMismatch):
        idx.search_mmr_arrays(np.zeros(7), 2, 4)
    with pytest.raises(V.IndexOpError, match="metric"):
        idx.search_mmr_arrays(q, 2, 4, 0.5, 7)
    for lam in (float("nan"), -0.1, 1.5):
        with pytest.raises(V.IndexOpError, match="lambda"):
            idx.search_mmr_arrays(q, 2, 4, lam)
    with pytest.raises(V.IndexOpError, match="fetch_k"):
        idx.search_mmr_arrays(q, 5, 4)
    with pytest.raises(V.IndexOpError, match="VL_MMR_MAX_FETCH"):
        idx.search_mmr_arrays(q, 5, 1025)
    f = idx.make_filter([1, 2])
    tok = f.token
    f.close()
    rc, _, _ = raw_call(idx, q, 2, 4, 0.5, COS, 4, token=tok)
    assert rc == 8  # VL_ERR_INVALID_ARG: a destroyed filter
    rc, _, _ = raw_call(idx, q, 2, 4, 0.5, COS, 4, token=(1 << 60))
    assert rc == 8
    empty = V.FlatIndex(8)
    gi, _ = empty.search_mmr_arrays(np.zeros(3), 2, 4)  # an empty index checks no dimension
    assert gi.size == 0
    hn = V.HNSWIndex(8)
    hn.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        hn.search_mmr_arrays(q, 2, 4)
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        hn.search_mmr(q, 2, 4)
    mi = V.MultiFlatIndex(8, [0, 0])
    mi.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        mi.search_mmr_arrays(q, 2, 4)


# ---- 6. concurrency ------------------------------------------------------------------------------
def test_eight_mmr_threads_beside_plain_searches(V, O):
    rng = np.random.default_rng(28)
    n, dim = 50_000, 64
    case = Case(V, O, dim, random_ids(rng, n), clustered(rng, n, dim))
    q = case.rows[31] + 0.02 * rng.standard_normal(dim)
    params = [(4, 20, 0.5), (10, 60, 0.25), (10, 61, 0.5), (50, 300, 0.0), (64, 1024, 0.5), (3, 10, 1.0), (20, 200, 0.75), (1, 1, 0.5)]
    lone = [case.idx.search_mmr_arrays(q, k, f, lam, COS) for k, f, lam in params]
    for (k, f, lam), (gi, gs) in zip(params, lone):
        ei, es, _ = case.expect(q, k, f, lam, COS)
        assert gi.tolist() == ei.tolist() and bits(gs) == bits(es)
    plain = case.idx.search_arrays(q, 10, COS)
    errors, stop = [], threading.Event()

    def mmr_worker(t):
        k, f, lam = params[t]
        try:
            for _ in range(25):
                gi, gs = case.idx.search_mmr_arrays(q, k, f, lam, COS)
                if gi.tolist() != lone[t][0].tolist() or bits(gs) != bits(lone[t][1]):
                    errors.append(("mmr", t))
                    return
        except Exception as e:  # noqa: BLE001
            errors.append(("mmr", t, repr(e)))

    def plain_worker():
        try:
            while not stop.is_set():
                gi, gs = case.idx.search_arrays(q, 10, COS)
                if gi.tolist() != plain[0].tolist() or bits(gs) != bits(plain[1]):
                    errors.append(("plain",))
                    return
        except Exception as e:  # noqa: BLE001
            errors.append(("plain", repr(e)))

    ninth = threading.Thread(target=plain_worker)
    ninth.start()
    threads = [threading.Thread(target=mmr_worker, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    stop.set()
    ninth.join()
    assert not errors, errors


# ---- 7. wrappers ---------------------------------------------------------------------------------
def test_wrappers_reattach_text_and_metadata(V, O):
    from vectorlite_amd import client as CL
    rng = np.random.default_rng(29)
    dim, n = 12, 200
    rows = clustered(rng, n, dim)

    class Embed:
        def __init__(self):
            self.table = {}

        def dimension(self):
            return dim

        def generate_embedding(self, text):
            return self.table[text]

    emb = Embed()
    cl = CL.VectorLiteClient(emb)
    cl.create_collection("docs", CL.IndexType.Flat)
    coll = cl.get_collection("docs")
    ids = []
    for i in range(n):
        emb.table["chunk %d" % i] = rows[i].tolist()
        ids.append(coll.add_text_with_metadata("chunk %d" % i, {"i": i}, emb))
    case = Case.__new__(Case)
    case.V, case.O, case.dim, case.ids, case.rows, case.idx, case._cand = V, O, dim, np.array(ids, dtype=np.uint64), rows, coll.index, {}
    case.ref = O.FlatOracle(dim, np.arange(n, dtype=np.uint64), rows)
    q = rows[3] + 0.02 * rng.standard_normal(dim)
    emb.table["question"] = q.tolist()
    ei, es, _ = case.expect(q, 5, 20, 0.5, COS)
    res = coll.index.search_mmr(q, 5, 20, 0.5, V.SimilarityMetric.Cosine)
    via_text = coll.search_text_mmr("question", 5, V.SimilarityMetric.Cosine, emb)  # defaults: fetch_k = 20, lambda_mult = 0.5
    for got in (res, via_text):
        assert [r.id for r in got] == ei.tolist() and bits([r.score for r in got]) == bits(es)
        assert all(isinstance(r, V.SearchResult) for r in got)
        assert [r.text for r in got] == ["chunk %d" % ids.index(int(i)) for i in ei]
        assert [r.metadata for r in got] == [{"i": ids.index(int(i))} for i in ei]
    wide = coll.search_text_mmr("question", 5, V.SimilarityMetric.Cosine, emb, fetch_k=50, lambda_mult=0.25)
    wi, ws, _ = case.expect(q, 5, 50, 0.25, COS)
    assert [r.id for r in wide] == wi.tolist() and bits([r.score for r in wide]) == bits(ws)
    rc, gi, gs = raw_call(coll.index, q, 5, 20, 0.5, COS, 5)  # the plain-C route, raw pointers
    assert rc == 0 and gi.tolist() == ei.tolist() and bits(gs) == bits(es)
