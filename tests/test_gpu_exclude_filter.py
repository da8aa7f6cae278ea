"""Exclusion id filters (vl_index_filter_create_excluding) against the oracle: every call that takes the
token answers exactly what FlatIndex::search gives on a FlatIndex that holds only the rows whose id is NOT in the set, in
storage order -- ids equal, f64 scores equal bit for bit -- and a single filtered search takes the masked ladder wherever its
route conditions hold."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, EUC, MAN, DOT = 0, 1, 2, 3
METRICS = (COS, EUC, MAN, DOT)
KFAST_MAX = 60
VL_ERR_INVALID_ARG = 8


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


@pytest.fixture
def no_floors(monkeypatch):
    """Handles created inside the test run the whole ladder at any size (the floors are read at create)."""
    monkeypatch.setenv("VL_SINGLE_FILTER_MIN_MB", "0")
    monkeypatch.setenv("VL_SINGLE_FILTER_I8_MIN_MB", "0")
    monkeypatch.delenv("VL_SINGLE_FILTER", raising=False)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64).tolist()


def random_ids(rng, n):
    """n distinct ids below 2^40 in random order (an odd multiplier is a bijection modulo 2^40)."""
    base = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(rng.integers(1 << 20))) % np.uint64(1 << 40)
    return rng.permutation(base)


def kept_mask(ids, excluded):
    return ~np.isin(ids, np.asarray(sorted(excluded), dtype=np.uint64)) if len(excluded) else np.ones(ids.size, bool)


def family(variant):
    """'f32' / 'bf16' / 'i8' for the variant code of a masked or an unmasked single-query scan; None for any other scan."""
    if variant <= 0:
        return None
    return {0: "f32", 1: "bf16", 2: "i8", 7: "f32", 8: "bf16", 9: "i8"}.get(variant // 1_000_000)


def masked(variant):
    return 7_000_000 <= variant < 10_000_000


def specialised(idx, q):
    """Does the library run a specialised f32 scan at this index's row stride (a VL_SCAN_VARIANTS entry)?  Asked of the
    library itself: an unfiltered f32-only search reports a negative variant for the run-time-stride kernel."""
    idx.set_single_filter("f32")  # (the caller sets its own mode afterwards)
    idx.search_arrays(q, 1, COS)
    return idx.last_scan()["variant"] > 0


def exclusion_sets(rng, ids):
    """Empty, one id, 10 ids, n / 100, n / 2, all but one row, every id, only ids the index lacks."""
    n = ids.size
    pick = lambda m: [int(x) for x in rng.choice(ids, size=min(max(m, 1), n), replace=False)]
    absent = [int(x) for x in (np.uint64(1 << 41) + np.arange(20, dtype=np.uint64))]
    return [[], pick(1), pick(10), pick(n // 100), pick(n // 2), [int(x) for x in ids[ids != ids[n // 3]]],
            [int(x) for x in ids], absent]


# ---- 1. parity and route ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16", "i8"])
# dim 3 and 50: run-time strides (the list route); 384 and 768: the kernel-argument query; 1024: a specialised stride past
# it (the masked f32 scan reads the f64 query from device memory; no int8 or bf16 query form there)
@pytest.mark.parametrize("dim", [3, 50, 384, 768, 1024])
def test_parity_with_the_oracle_over_the_kept_rows(V, O, no_floors, dim, mode):
    rng = np.random.default_rng(7000 + dim)
    routed, special = 0, None
    for n in (1, 63, 64, 65, 4133, 20_000):
        ids = random_ids(rng, n)
        rows = rng.standard_normal((n, dim))
        idx = V.FlatIndex(dim)
        idx.add_rows(ids, rows, validate=False)
        q = rng.standard_normal(dim)
        special = specialised(idx, q)
        idx.set_single_filter(mode)
        assert special == (dim in (384, 768, 1024)), "construction: which dims the route conditions hold at"
        for excluded in exclusion_sets(rng, ids):
            keep = kept_mask(ids, excluded)
            m = int(keep.sum())
            ref = O.FlatOracle(dim, ids[keep], rows[keep])
            with idx.make_filter(excluded, exclude=True) as f:
                assert f.exclude and f.rows() == m
                for metric in METRICS:
                    ri, rs = ref.search(q, m, metric) if m else (np.zeros(0, np.uint64), np.zeros(0))  # every k is a prefix
                    for k in (1, 10, 60, 61, m + 5):
                        gi, gs = idx.search_arrays(q, k, metric, exclude=f)
                        ctx = (dim, n, len(excluded), metric, k, mode)
                        assert gi.tolist() == ri[:k].tolist(), ctx
                        assert bits(gs) == bits(rs[:k]), ctx
                        if m and min(k, m) <= KFAST_MAX and special:
                            # the route conditions hold (gaussian rows and query are in the fast-path domain)
                            assert masked(idx.last_scan()["variant"]), (ctx, idx.last_scan())
                            routed += 1
                        elif m and not special:  # a generic stride never sees a masked scan (the list route)
                            assert not masked(idx.last_scan()["variant"]), (ctx, idx.last_scan())
    assert (routed > 0) == special


def test_one_shot_ids_equal_the_token(V, O):
    rng = np.random.default_rng(3)
    n, dim = 4133, 384
    ids = random_ids(rng, n)
    ids[100:110] = ids[2000]  # duplicate-id rows: all of them are excluded together
    rows = rng.standard_normal((n, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    q = rows[2000] + 0.01 * rng.standard_normal(dim)
    excluded = [int(ids[2000])] + [int(x) for x in ids[::7]]
    keep = kept_mask(ids, excluded)
    ref = O.FlatOracle(dim, ids[keep], rows[keep])
    ri, rs = ref.search(q, 30, COS)
    # unsorted, repeated and absent ids change nothing
    shuffled = [int(x) for x in rng.permutation(excluded)] + excluded[:20] + [1 << 45, (1 << 45) + 1]
    for ex in (excluded, shuffled):
        gi, gs = idx.search_arrays(q, 30, COS, exclude=ex)
        assert gi.tolist() == ri.tolist() and bits(gs) == bits(rs)
    assert int(ids[2000]) not in idx.search_arrays(q, 30, COS, exclude=excluded)[0].tolist()
    res = idx.search(q, 5, exclude=excluded)
    assert [r.id for r in res] == ri[:5].tolist()


# ---- 2. stage determinism ----------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [384, 768])
def test_masked_ladder_ends_in_the_stage_the_unmasked_one_does(V, no_floors, dim):
    """The largest-norm row is kept, so the masked call and the unmasked search on an index of the kept rows see the same
    lists, n_rows and norm bound: the certificate's outcome, and with it the last stage, is the same.  No tolerance."""
    rng = np.random.default_rng(90 + dim)
    n = 20_000
    rows = rng.standard_normal((n, dim)) * rng.uniform(0.5, 2.0, size=(n, 1))
    # near-duplicates no int8 or bf16 key can tell apart: queries next to them walk down the ladder
    b = rng.choice([-1.0, 1.0], size=dim) / np.sqrt(dim)
    rows[5000:5150] = b[None, :] * (1.0 + 2.0 ** -20 * np.arange(150)[:, None])
    ids = random_ids(rng, n)
    big = int(np.argmax(np.linalg.norm(rows, axis=1)))
    out = rng.choice(np.setdiff1d(np.arange(n), [big]), size=n // 100, replace=False)
    keep = np.ones(n, bool)
    keep[out] = False
    full, part = V.FlatIndex(dim), V.FlatIndex(dim)
    full.add_rows(ids, rows, validate=False)
    part.add_rows(ids[keep], rows[keep], validate=False)
    queries = [rng.standard_normal(dim) for _ in range(3)] + [b + 0.01 * rng.standard_normal(dim) / np.sqrt(dim)]
    seen = set()
    with full.make_filter([int(x) for x in ids[out]], exclude=True) as f:
        for mode in ("auto", "i8", "bf16", "f32"):
            full.set_single_filter(mode)
            part.set_single_filter(mode)
            for metric in (COS, DOT):
                for q in queries:
                    pi, ps = part.search_arrays(q, 10, metric)
                    want, want_path = family(part.last_scan()["variant"]), V.last_path()
                    gi, gs = full.search_arrays(q, 10, metric, exclude=f)
                    got, got_path = full.last_scan()["variant"], V.last_path()
                    assert gi.tolist() == pi.tolist() and bits(gs) == bits(ps)
                    # the same last stage and the same route out of it: certified there, or (both) on to the exact
                    # kernels behind the f32 stage
                    assert got_path == want_path, (mode, metric, got_path, want_path, got, part.last_scan())
                    assert masked(got) and family(got) == want, (mode, metric, got, part.last_scan())
                    seen.add((want, want_path))
    # otherwise the comparison proves nothing: every stage certified some query
    assert {(s, V.PATH_FAST) for s in ("i8", "bf16", "f32")} <= seen, seen


# ---- 3. correctness under stress -------------------------------------------------------------------
def test_excluded_near_duplicates_at_the_top(V, O, no_floors):
    rng = np.random.default_rng(17)
    n, dim = 20_000, 384
    rows = rng.standard_normal((n, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    q = rng.standard_normal(dim)
    q /= np.linalg.norm(q)
    where = np.sort(rng.choice(n, size=100, replace=False))
    rows[where] = q[None, :] + 1e-6 * rng.standard_normal((100, dim))  # the query's best 100 rows
    ids = random_ids(rng, n)
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    keep = np.ones(n, bool)
    keep[where] = False
    ref = O.FlatOracle(dim, ids[keep], rows[keep])
    with idx.make_filter([int(x) for x in ids[where]], exclude=True) as f:
        for metric in METRICS:
            ri, rs = ref.search(q, 61, metric)
            for k in (1, 10, 60, 61):
                gi, gs = idx.search_arrays(q, k, metric, exclude=f)
                assert gi.tolist() == ri[:k].tolist() and bits(gs) == bits(rs[:k]), (metric, k)
                assert not np.isin(gi, ids[where]).any()


def test_nan_row_counts_only_when_kept(V, O):
    rng = np.random.default_rng(19)
    n, dim = 1000, 384
    ids = np.arange(n, dtype=np.uint64)
    rows = rng.standard_normal((n, dim))
    rows[500, 3] = np.nan
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    q = rng.standard_normal(dim)
    ref = O.FlatOracle(dim, ids[ids != 500], rows[ids != 500])
    for metric in METRICS:
        ri, rs = ref.search(q, 10, metric)
        gi, gs = idx.search_arrays(q, 10, metric, exclude=[500])
        assert gi.tolist() == ri.tolist() and bits(gs) == bits(rs)
        with pytest.raises(V.NaNScore):
            idx.search_arrays(q, 10, metric, exclude=[7])
        with pytest.raises(V.NaNScore):
            idx.search_arrays(q, 10, metric, exclude=[])


# ---- 4. staleness and lifetime -------------------------------------------------------------------------
def test_token_follows_adds_and_deletes(V, O):
    rng = np.random.default_rng(23)
    n, dim = 4133, 384
    ids = np.arange(n, dtype=np.uint64) * np.uint64(2)
    rows = rng.standard_normal((n, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    excluded = [int(x) for x in ids[1::3]] + [20_001, 20_003]  # two ids the index does not hold yet
    q = rng.standard_normal(dim)
    f = idx.make_filter(excluded, exclude=True)

    def agree():
        eids, evals = idx.export()
        keep = kept_mask(eids, excluded)
        assert f.rows() == int(keep.sum())
        ref = O.FlatOracle(dim, eids[keep], evals[keep])
        for metric in (COS, MAN):
            for k in (10, 61):
                ri, rs = ref.search(q, k, metric)
                gi, gs = idx.search_arrays(q, k, metric, exclude=f)
                assert gi.tolist() == ri.tolist() and bits(gs) == bits(rs)

    agree()
    idx.add(V.Vector(id=20_001, values=list(q * 1.5)))  # an excluded id arrives: the best row, and it stays out
    agree()
    assert 20_001 not in idx.search_arrays(q, 5, COS, exclude=f)[0].tolist()
    idx.add_rows(np.array([20_005, 20_007], dtype=np.uint64), np.stack([q * 1.25, rng.standard_normal(dim)]))  # fresh ids
    agree()
    assert idx.search_arrays(q, 1, COS, exclude=f)[0].tolist() == [20_005]
    for d in (int(ids[0]), int(ids[1]), 20_005):
        idx.delete(d)
        agree()
    idx.delete_many([int(x) for x in ids[10:400]] + [20_001])
    agree()
    f.close()


def test_clone_destroyed_token_and_refusing_handles(V):
    rng = np.random.default_rng(29)
    n, dim = 500, 384
    idx = V.FlatIndex(dim)
    idx.add_rows(np.arange(n, dtype=np.uint64), rng.standard_normal((n, dim)), validate=False)
    q = rng.standard_normal(dim)
    f = idx.make_filter([1, 2, 3], exclude=True)
    assert f.token != 0 and f.rows() == n - 3
    g = idx.make_filter([1, 2, 3])
    assert g.token not in (0, f.token) and not g.exclude  # one token space
    twin = idx.clone()
    out_ids, out_scores, out_n = np.zeros(10, np.uint64), np.zeros(10), C.c_uint64(0)
    raw = lambda index, tok: index._L.vl_index_search_filtered(index._h, tok, q.ctypes.data, q.size, 10, COS, 10, out_ids.ctypes.data,
                                                               out_scores.ctypes.data, C.byref(out_n))
    assert raw(idx, f.token) == 0 and out_n.value == 10
    assert raw(twin, f.token) == VL_ERR_INVALID_ARG  # a clone does not copy tokens
    tok = f.token
    f.close()
    assert raw(idx, tok) == VL_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        idx.search_arrays(q, 10, COS, filter=g, exclude=[1])
    with pytest.raises(ValueError):
        idx.search_batch(q[None, :], 10, COS, filter=[1], exclude=[2])
    with pytest.raises(ValueError):
        idx.search_arrays(q, 10, COS, exclude=g)  # an include token is not an exclusion
    # dimension and metric errors are the include filter's
    with idx.make_filter([1], exclude=True) as h:
        with pytest.raises(V.DimensionMismatch):
            idx.search_arrays(q[:-1], 10, COS, exclude=h)
        with pytest.raises((V.IndexOpError, V.VectorLiteError)):
            idx.search_arrays(q, 10, 9, exclude=h)
        assert idx.search_arrays(q, 0, COS, exclude=h)[0].size == 0
    hn = V.HNSWIndex(dim, COS)
    with pytest.raises(V.IndexOpError):
        hn.make_filter([1], exclude=True)
    with pytest.raises(V.IndexOpError):
        hn.search(q, 5, COS, exclude=[1])
    multi = V.MultiFlatIndex(dim, devices=[0])
    with pytest.raises(V.IndexOpError):
        multi.make_filter([1], exclude=True)


# ---- 5. the list-route consumers ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def consumer_case(V, O):
    rng = np.random.default_rng(31)
    n, dim = 4133, 384
    ids = random_ids(rng, n)
    centres = rng.standard_normal((40, dim))
    rows = centres[rng.integers(40, size=n)] + 0.3 * rng.standard_normal((n, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    excluded = [int(x) for x in rng.choice(ids, size=n // 3, replace=False)]
    keep = kept_mask(ids, excluded)
    positions = np.nonzero(keep)[0].astype(np.uint64)
    ref = O.FlatOracle(dim, positions, rows[keep])  # ids = storage positions
    return {"idx": idx, "ids": ids, "rows": rows, "excluded": excluded, "keep": keep, "ref": ref, "rng": rng, "dim": dim,
            "m": int(keep.sum())}


def test_search_batch_mixes_both_kinds_of_token(V, O, consumer_case):
    c = consumer_case
    idx, ids, rows, rng = c["idx"], c["ids"], c["rows"], c["rng"]
    Q = rng.standard_normal((6, c["dim"]))
    include = [int(x) for x in ids[::5]]
    inc_ref = O.FlatOracle(c["dim"], ids[::5], rows[::5])
    with idx.make_filter(c["excluded"], exclude=True) as fe, idx.make_filter(include) as fi:
        gi, gs, gn = idx.search_batch(Q, 10, COS, filters=[fe, fi, fe, fi, fe, fe])
        for j, f in enumerate((fe, fi, fe, fi, fe, fe)):
            if f is fe:
                rp, rs = c["ref"].search(Q[j], 10, COS)
                ri = ids[rp.astype(np.int64)]
            else:
                ri, rs = inc_ref.search(Q[j], 10, COS)
            assert gn[j] == 10 and gi[j].tolist() == ri.tolist() and bits(gs[j]) == bits(rs), j
        gi, gs, gn = idx.search_batch(Q, 10, DOT, exclude=fe)  # one exclusion token for the batch
        for j in range(6):
            rp, rs = c["ref"].search(Q[j], 10, DOT)
            assert gi[j].tolist() == ids[rp.astype(np.int64)].tolist() and bits(gs[j]) == bits(rs), j


def test_range_search_and_its_batch(V, O, consumer_case):
    c = consumer_case
    idx, ids, rng = c["idx"], c["ids"], c["rng"]
    Q = rng.standard_normal((3, c["dim"]))
    want = []
    for q in Q:
        rp, rs = c["ref"].search(q, c["m"], COS)
        t = float(rs[25])  # a threshold that sits on a score
        cut = int((rs >= t).sum())
        want.append((t, ids[rp[:cut].astype(np.int64)].tolist(), bits(rs[:cut])))
        gi, gs, total = idx.search_range_arrays(q, t, COS, exclude=c["excluded"])
        assert total == cut and gi.tolist() == want[-1][1] and bits(gs) == want[-1][2]
    li, ls, totals = idx.search_range_batch_arrays(Q, [w[0] for w in want], COS, exclude=c["excluded"])
    for j, w in enumerate(want):
        assert totals[j] == len(w[1]) and li[j].tolist() == w[1] and bits(ls[j]) == w[2], j


def test_mmr_search(V, O, consumer_case):
    from test_gpu_mmr_search import mmr_reference
    c = consumer_case
    idx, ids, rows = c["idx"], c["ids"], c["rows"]
    q = rows[77] + 0.02 * c["rng"].standard_normal(c["dim"])
    for fetch_k in (20, 100):
        rp, rs = c["ref"].search(q, fetch_k, COS)
        cand = rows[rp.astype(np.int64)]
        sel = mmr_reference(O, COS, rs.tolist(), cand, 8, 0.5, {})
        gi, gs = idx.search_mmr_arrays(q, 8, fetch_k, 0.5, COS, exclude=c["excluded"])
        assert gi.tolist() == ids[rp[sel].astype(np.int64)].tolist() and bits(gs) == bits(rs[sel]), fetch_k


def test_grouped_search(V, O, consumer_case):
    c = consumer_case
    idx, ids = c["idx"], c["ids"]
    gkeys = (np.arange(ids.size, dtype=np.uint64) % np.uint64(300)) * np.uint64(0x9E3779B97F4A7C15)
    table = idx.make_groups(ids, gkeys)
    q = c["rng"].standard_normal(c["dim"])
    rp, rs = c["ref"].search(q, c["m"], COS)
    seen, ek, ei, es = set(), [], [], []
    for p, s in zip(rp.tolist(), rs.tolist()):  # the ranking of the kept rows, collapsed to the first row of each group
        g = int(gkeys[p])
        if g not in seen:
            seen.add(g)
            ek.append(g)
            ei.append(int(ids[p]))
            es.append(s)
    gk, gi, gs = idx.search_grouped_arrays(q, 10, COS, groups=table, exclude=c["excluded"])
    assert gk.tolist() == ek[:10] and gi.tolist() == ei[:10] and bits(gs) == bits(es[:10])
    table.close()


# ---- 6. concurrency ------------------------------------------------------------------------------------
def test_four_threads_one_token(V, O, consumer_case):
    c = consumer_case
    idx, ids = c["idx"], c["ids"]
    Q = c["rng"].standard_normal((8, c["dim"]))
    with idx.make_filter(c["excluded"], exclude=True) as f:
        alone = [idx.search_arrays(q, k, COS, exclude=f) for q in Q for k in (10, 61)]
        rp, rs = c["ref"].search(Q[0], 10, COS)
        assert alone[0][0].tolist() == ids[rp.astype(np.int64)].tolist() and bits(alone[0][1]) == bits(rs)
        errors = []

        def worker():
            try:
                for _ in range(5):
                    got = [idx.search_arrays(q, k, COS, exclude=f) for q in Q for k in (10, 61)]
                    for a, b in zip(alone, got):
                        assert a[0].tolist() == b[0].tolist() and bits(a[1]) == bits(b[1])
            except Exception as e:  # noqa: BLE001 (reported on the main thread)
                errors.append(e)

        threads = [threading.Thread(target=worker) for _ in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
