"""Search restricted to an id filter (vl_index_filter_* / vl_index_search_filtered) against the oracle: the answer is
exactly FlatIndex::search on a FlatIndex that holds only the rows whose id is in the set, in storage order -- ids equal,
f64 scores equal bit for bit."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, EUC, MAN, DOT = 0, 1, 2, 3
SUBSET_VARIANT_BASE = 3_000_000


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


def oracle_answer(O, dim, ids, rows, keep, q, k, metric):
    """The reference's answer over the rows whose id is in `keep`, in storage order."""
    sel = np.isin(ids, np.asarray(sorted(keep), dtype=np.uint64)) if len(keep) else np.zeros(ids.size, bool)
    ref = O.FlatOracle(dim, ids[sel], rows[sel])
    ri, rs = ref.search(q, k, metric)
    return ri.tolist(), bits(rs)


def subset_oracle(O, dim, ids, rows, keep):
    sel = np.isin(ids, np.asarray(sorted(keep), dtype=np.uint64)) if len(keep) else np.zeros(ids.size, bool)
    return O.FlatOracle(dim, ids[sel], rows[sel])


def check(V, O, idx, dim, ids, rows, keep, q, k, metric, filt=None, ref=None):
    gi, gs = idx.search_arrays(q, k, metric, filter=filt if filt is not None else list(keep))
    if ref is None:
        ri, rs = oracle_answer(O, dim, ids, rows, keep, q, k, metric)
    else:
        ri, rs = ref.search(q, k, metric)
        ri, rs = ri.tolist(), bits(rs)
    assert gi.tolist() == ri, (dim, len(keep), k, metric)
    assert bits(gs) == rs, (dim, len(keep), k, metric)


def random_ids(rng, n):
    """n distinct ids below 2^40 in random order (an odd multiplier is a bijection modulo 2^40)."""
    base = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(rng.integers(1 << 20))) % np.uint64(1 << 40)
    return rng.permutation(base)


def subsets(rng, ids):
    n = ids.size
    out = [[], [int(ids[rng.integers(n)])]]
    for m in (10, max(1, n // 100), n // 2, n):
        m = min(m, n)
        out.append([int(x) for x in rng.choice(ids, size=m, replace=False)])
    return out


@pytest.mark.parametrize("dim,sizes", [(3, (1, 63, 64, 65, 10_000)), (50, (1, 64, 65, 10_000, 200_000)),
                                       (384, (1, 63, 65, 10_000, 200_000)), (768, (1, 64, 10_000))])
def test_parity_with_the_oracle_over_the_subset(V, O, dim, sizes):
    rng = np.random.default_rng(dim)
    for n in sizes:
        ids = random_ids(rng, n)
        rows = rng.standard_normal((n, dim))
        idx = V.FlatIndex(dim)
        idx.add_rows(ids, rows, validate=False)
        q = rng.standard_normal(dim)
        for keep in subsets(rng, ids):
            ref = subset_oracle(O, dim, ids, rows, keep)
            with idx.make_filter(keep) as f:
                assert f.rows() == len(set(keep))
                m = len(set(keep))
                for metric in (COS, EUC, MAN, DOT):
                    for k in (1, 10, 60, 61, 200, m + 5):
                        if n >= 200_000 and k == 200 and metric == MAN:
                            continue  # the 200-row exact selection is covered at every other shape; keep the file short
                        check(V, O, idx, dim, ids, rows, keep, q, k, metric, filt=f, ref=ref)


def test_full_filter_equals_the_unfiltered_search(V):
    rng = np.random.default_rng(11)
    n, dim = 20_000, 384
    ids = random_ids(rng, n)
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rng.standard_normal((n, dim)), validate=False)
    with idx.make_filter(ids) as f:
        for metric in (COS, EUC, MAN, DOT):
            for k in (1, 10, 60, 100):
                q = rng.standard_normal(dim)
                a = idx.search_arrays(q, k, metric)
                b = idx.search_arrays(q, k, metric, filter=f)
                assert a[0].tolist() == b[0].tolist() and bits(a[1]) == bits(b[1])


def test_id_set_rules(V, O):
    rng = np.random.default_rng(5)
    n, dim = 3000, 50
    ids = random_ids(rng, n)
    ids[100:110] = ids[2000]  # duplicate-id rows: all of them qualify
    rows = rng.standard_normal((n, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    q = rng.standard_normal(dim)
    keep = [int(ids[2000])] + [int(x) for x in ids[::7]]
    absent = [int(x) for x in (np.uint64(1 << 41) + np.arange(50, dtype=np.uint64))]
    with idx.make_filter(keep) as f:
        assert f.rows() == int(np.isin(ids, np.asarray(keep, dtype=np.uint64)).sum())
        for metric in (COS, EUC, DOT):
            check(V, O, idx, dim, ids, rows, keep, q, 30, metric, filt=f)
            base = idx.search_arrays(q, 30, metric, filter=f)
            # unsorted, repeated and absent ids change nothing
            shuffled = list(rng.permutation(keep)) + keep[:20] + absent
            other = idx.search_arrays(q, 30, metric, filter=shuffled)
            assert base[0].tolist() == other[0].tolist() and bits(base[1]) == bits(other[1])
    with idx.make_filter(absent) as f:
        assert f.rows() == 0
        assert idx.search_arrays(q, 10, COS, filter=f)[0].size == 0


def test_ties_resolve_by_position(V, O):
    rng = np.random.default_rng(9)
    n, dim = 5000, 384
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    q = rng.standard_normal(dim)
    twin = q * 3.0
    planted = [10, 400, 401, 2500, 4999]  # equal best rows, some inside the subset and some outside
    rows[planted] = twin
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    keep = [int(ids[p]) for p in (400, 2500, 4999)] + [int(x) for x in ids[::5]]
    for metric in (COS, EUC, MAN, DOT):
        for k in (1, 3, 10):
            check(V, O, idx, dim, ids, rows, keep, q, k, metric)


def test_fast_path_reads_only_the_subset_rows(V, O):
    rng = np.random.default_rng(1)
    n, dim = 200_000, 384
    ids = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    rows = rng.standard_normal((n, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    keep = [int(x) for x in rng.choice(ids, size=n // 10, replace=False)]
    m = len(keep)
    with idx.make_filter(keep) as f:
        for metric in (COS, DOT):
            q = rng.standard_normal(dim)
            q /= np.linalg.norm(q)
            idx.search_arrays(q, 10, metric, filter=f)  # warm
            idx.profile_read()
            idx.profile_enable(True)
            gi, gs = idx.search_arrays(q, 10, metric, filter=f)
            idx.profile_enable(False)
            nl, _, by = idx.profile_read()
            assert V.last_path() == V.PATH_FAST
            assert SUBSET_VARIANT_BASE <= idx.last_scan()["variant"] < SUBSET_VARIANT_BASE + 1_000_000
            assert nl == 1 and by <= 1.05 * (m * dim * 4 + 8 * m) and by < n * dim * 4 / 5
            ri, rs = oracle_answer(O, dim, ids, rows, keep, q, 10, metric)
            assert gi.tolist() == ri and bits(gs) == rs


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


def test_exact_fallback_and_forced_paths(V, O):
    rng = np.random.default_rng(3)
    n, dim = 40_000, 384
    rows, q, where = near_duplicates(rng, n, dim)
    ids = np.arange(n, dtype=np.uint64) + np.uint64(100)
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    keep = [int(ids[p]) for p in where] + [int(x) for x in ids[::4]]
    with idx.make_filter(keep) as f:
        for metric in (COS, EUC, DOT):
            for k in (10, 60):
                check(V, O, idx, dim, ids, rows, keep, q, k, metric, filt=f)
                for path in (V.PATH_EXACT_SELECT, V.PATH_EXACT_SORT):
                    idx.force_path(path)
                    try:
                        check(V, O, idx, dim, ids, rows, keep, q, k, metric, filt=f)
                        assert V.last_path() == path
                    finally:
                        idx.force_path(0)


def test_nan_only_counts_inside_the_subset(V):
    rng = np.random.default_rng(4)
    n, dim = 1000, 16
    ids = np.arange(n, dtype=np.uint64)
    rows = rng.standard_normal((n, dim))
    rows[500, 3] = np.nan
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    q = rng.standard_normal(dim)
    outside = [int(x) for x in ids if x != 500]
    gi, _ = idx.search_arrays(q, 10, COS, filter=outside)
    assert gi.size == 10
    with pytest.raises(V.NaNScore):
        idx.search_arrays(q, 10, COS, filter=[1, 2, 500, 7])
    gi, gs = idx.search_arrays(q, 10, COS, filter=[500])  # a 1-row sort never compares: its score is returned
    assert gi.tolist() == [500] and np.isnan(gs[0])


def test_filter_follows_adds_and_deletes(V, O):
    rng = np.random.default_rng(6)
    n, dim = 5000, 64
    ids = np.arange(n, dtype=np.uint64) * np.uint64(2)
    rows = rng.standard_normal((n, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    keep = [int(x) for x in ids[1::3]] + [20_001, 20_003, 20_005]  # three ids that arrive later
    q = rng.standard_normal(dim)
    f = idx.make_filter(keep)
    assert f.rows() == len(ids[1::3])

    def state():
        eids, evals = idx.export()
        return eids, evals

    def agree():
        eids, evals = state()
        assert f.rows() == int(np.isin(eids, np.asarray(keep, dtype=np.uint64)).sum())
        for metric in (COS, EUC):
            check(V, O, idx, dim, eids, evals, keep, q, 10, metric, filt=f)

    agree()
    idx.add(V.Vector(id=20_001, values=list(rng.standard_normal(dim))))
    agree()
    idx.add_rows(np.array([20_003, 20_005, 20_007], dtype=np.uint64), rng.standard_normal((3, dim)))
    agree()
    for d in (int(ids[0]), int(ids[4]), int(ids[1]), 20_003):  # deletes in front of allowed rows shift their positions
        idx.delete(d)
        agree()
    f.close()


def test_errors(V):
    rng = np.random.default_rng(8)
    idx = V.FlatIndex(8)
    idx.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    with idx.make_filter([1 << 50]) as f:  # empty subset: the dimension check still runs
        with pytest.raises(V.DimensionMismatch):
            idx.search_arrays(np.zeros(7), 3, COS, filter=f)
        assert idx.search_arrays(np.zeros(8), 3, COS, filter=f)[0].size == 0
    with idx.make_filter([1, 2]) as f:
        assert idx.search_arrays(np.zeros(8), 0, COS, filter=f)[0].size == 0
        with pytest.raises(V.IndexOpError):
            idx.search_arrays(np.zeros(8), 3, 7, filter=f)  # unknown metric
    f = idx.make_filter([1, 2])
    tok = f.token
    f.close()
    L = idx._L
    import ctypes as C
    n = C.c_uint64(0)
    q = np.zeros(8)
    out_i, out_s = np.zeros(4, dtype=np.uint64), np.zeros(4)
    rc = L.vl_index_search_filtered(idx._h, tok, q.ctypes.data, 8, 3, 0, 4, out_i.ctypes.data,
                                    out_s.ctypes.data, C.addressof(n))
    assert rc == 8
    hn = V.HNSWIndex(8)
    hn.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        hn.make_filter([1])
    mi = V.MultiFlatIndex(8, [0, 0])
    mi.add_rows(np.arange(10, dtype=np.uint64), rng.standard_normal((10, 8)))
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        mi.search_arrays(q, 3, COS, filter=[1, 2])
    # destroying a filter that was never there, or twice
    assert L.vl_index_filter_destroy(idx._h, 1 << 62) == 8


def test_concurrent_searches_share_one_stale_filter(V):
    rng = np.random.default_rng(12)
    n, dim = 50_000, 128
    ids = np.arange(n, dtype=np.uint64)
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rng.standard_normal((n, dim)), validate=False)
    keep = [int(x) for x in ids[::3]]
    f = idx.make_filter(keep)
    q = rng.standard_normal(dim)
    idx.delete(3)  # the filter is stale: the first searcher resolves it again
    idx.add(V.Vector(id=n + 1, values=list(rng.standard_normal(dim))))
    clone = idx.clone()
    with clone.make_filter(keep) as cf:
        lone = clone.search_arrays(q, 10, COS, filter=cf)
    out = [None] * 16

    def run(i):
        out[i] = idx.search_arrays(q, 10, COS, filter=f)

    th = [threading.Thread(target=run, args=(i,)) for i in range(16)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for r in out:
        assert r[0].tolist() == lone[0].tolist() and bits(r[1]) == bits(lone[1])
    f.close()


def test_batch_equals_single_filtered_searches(V):
    rng = np.random.default_rng(13)
    n, dim = 30_000, 384
    ids = np.arange(n, dtype=np.uint64)
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rng.standard_normal((n, dim)), validate=False)
    Q = rng.standard_normal((9, dim))
    with idx.make_filter(ids[::10]) as f:
        for metric in (COS, MAN):
            bi, bs, bn = idx.search_batch(Q, 12, metric, filter=f)
            for r in range(Q.shape[0]):
                si, ss = idx.search_arrays(Q[r], 12, metric, filter=f)
                assert int(bn[r]) == si.size
                assert bi[r, : si.size].tolist() == si.tolist() and bits(bs[r, : si.size]) == bits(ss)


def test_collection_search_text_where(V, O):
    from vectorlite_amd import client

    class Embedder:
        def __init__(self):
            self.rng = np.random.default_rng(14)

        def generate_embedding(self, text):
            return list(np.random.default_rng(abs(hash(text)) % (1 << 32)).standard_normal(16))

        def dimension(self):
            return 16

    cl = client.VectorLiteClient(Embedder())
    cl.create_collection("docs", client.IndexType.Flat)
    for i in range(300):
        cl.add_text_to_collection("docs", f"text {i}", {"user": i % 7})
    c = cl.get_collection("docs")
    where = lambda md: md["user"] == 3  # noqa: E731
    res = cl.search_text_in_collection("docs", "query", 5, V.SimilarityMetric.Cosine, where=where)
    eids, evals = c.index.export()
    keep = [i for i in eids.tolist() if i % 7 == 3]
    q = np.asarray(Embedder().generate_embedding("query"))
    ri, rs = oracle_answer(O, 16, eids, evals, keep, q, 5, COS)
    assert [r.id for r in res] == ri and bits([r.score for r in res]) == rs
    assert all(r.metadata == {"user": 3} and r.text == f"text {r.id}" for r in res)
    plain = cl.search_text_in_collection("docs", "query", 5)
    assert [r.id for r in plain] == c.index.search_arrays(q, 5, COS)[0].tolist()


def test_headline_size_fast_equals_exact(V, O):
    """10 M x 384 cosine from device embeddings: 0.1 % and 10 % subsets, fast answer = forced exact answer (= oracle at 0.1 %)."""
    import torch
    n, dim = 10_000_000, 384
    idx = V.FlatIndex(dim)
    idx.reserve(n)
    rng = np.random.default_rng(22)
    keeps = {frac: np.sort(rng.choice(n, size=int(n * frac), replace=False)).astype(np.uint64) for frac in (0.001, 0.1)}
    small = keeps[0.001].astype(np.int64)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(21)
    step = 2_500_000
    parts = []
    for lo in range(0, n, step):
        e = torch.randn((step, dim), dtype=torch.float32, device="cuda:0", generator=g)
        # f32 model output widened to f64 (exact): the oracle's rows of the 0.1 % subset are these values
        idx.add_embeddings(np.arange(lo, lo + step, dtype=np.uint64), e, normalize=False, validate=False)
        loc = small[(small >= lo) & (small < lo + step)] - lo
        parts.append(e[torch.from_numpy(loc).to("cuda:0")].double().cpu().numpy())
        del e
    torch.cuda.synchronize()
    small_rows = np.concatenate(parts)
    q = rng.standard_normal(dim)
    q /= np.linalg.norm(q)
    for frac, keep in keeps.items():
        with idx.make_filter(keep) as f:
            fi, fs = idx.search_arrays(q, 10, COS, filter=f)
            assert V.last_path() == V.PATH_FAST
            idx.force_path(V.PATH_EXACT_SELECT)
            try:
                ei, es = idx.search_arrays(q, 10, COS, filter=f)
            finally:
                idx.force_path(0)
            assert fi.tolist() == ei.tolist() and bits(fs) == bits(es)
            if frac == 0.001:
                ref = O.FlatOracle(dim, keep, small_rows)
                ri, rs = ref.search(q, 10, COS)
                assert fi.tolist() == ri.tolist() and bits(fs) == bits(rs)
