"""Attribute columns and predicate filter tokens (vl_index_attr_create / vl_index_filter_create_where)
against the oracle: every call that takes the token answers exactly what FlatIndex::search gives on a FlatIndex that holds
only the rows whose attribute values pass the clauses, in storage order -- ids equal, f64 scores equal bit for bit -- which
is also what the include token over the same rows answers, on the list route, the masked ladder and under "auto"."""
import ctypes as C
import threading

import numpy as np
import pytest

from test_gpu_exclude_filter import COS, DOT, EUC, KFAST_MAX, MAN, METRICS, VL_ERR_INVALID_ARG, bits, family, masked, random_ids, specialised

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


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


def column_values(rng, n):
    """(has, values): about one row in seven has no value; the others carry a permutation of -n//2 .. with the int64
    extremes on two of them when there is room."""
    has = (np.arange(n) % 7) != 3
    values = (rng.permutation(n).astype(np.int64) - n // 2)
    if n > 10:
        values[np.nonzero(has)[0][0]] = I64_MIN
        values[np.nonzero(has)[0][-1]] = I64_MAX
    return has, values


def passes(has, values, lo, hi, negate=False):
    lo = I64_MIN if lo is None else lo
    hi = I64_MAX if hi is None else hi
    return has & (((values >= lo) & (values <= hi)) != bool(negate))


def predicates(n, has, values):
    """Clauses keeping nothing, one row, ~1 %, ~50 %, all but one row (of those with a value), every row with a value."""
    one = int(values[np.nonzero(has)[0][len(np.nonzero(has)[0]) // 2]])
    return [(5, 4), (one, one), (-(n // 2), -(n // 2) + max(n // 100, 1)), (0, None), (one, one, True), (None, None), (7, 3, 1)]


def check_search(idx, f, inc, ref, ids_kept, q, m, ctx):
    """Every metric and k: the predicate token == the oracle over the qualifying rows == the include token."""
    for metric in METRICS:
        ri, rs = ref.search(q, m, metric) if m else (np.zeros(0, np.uint64), np.zeros(0))  # every k is a prefix
        for k in (1, 10, 60, 61, m + 5):
            gi, gs = idx.search_arrays(q, k, metric, filter=f)
            yield metric, k
            assert gi.tolist() == ri[:k].tolist(), (ctx, metric, k)
            assert bits(gs) == bits(rs[:k]), (ctx, metric, k)
            if inc is not None:
                ii, isc = idx.search_arrays(q, k, metric, filter=inc)
                assert ii.tolist() == gi.tolist() and bits(isc) == bits(gs), (ctx, metric, k, "include token")


# ---- 1. parity and routes --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16", "i8"])
@pytest.mark.parametrize("dim", [3, 50, 384, 768])
def test_parity_with_the_oracle_and_the_include_token(V, O, no_floors, dim, mode):
    rng = np.random.default_rng(8000 + dim)
    masked_seen = {"list": 0, "mask": 0}
    special = None
    for n in (1, 63, 64, 65, 4133, 20_000):
        ids = random_ids(rng, n)
        rows = rng.standard_normal((n, dim))
        idx = V.FlatIndex(dim)
        idx.add_rows(ids, rows, validate=False)
        q = rng.standard_normal(dim)
        special = specialised(idx, q)
        idx.set_single_filter(mode)
        assert special == (dim in (384, 768)), "construction: which dims the ladder's conditions hold at"
        has, values = column_values(rng, n)
        with idx.make_attribute(ids[has], values[has]) as col:
            assert col.rows() == int(has.sum())
            for clause in predicates(n, has, values):
                keep = passes(has, values, *clause)
                m = int(keep.sum())
                ref = O.FlatOracle(dim, ids[keep], rows[keep])
                with idx.make_filter_where([(col,) + tuple(clause)]) as f, idx.make_filter(ids[keep]) as inc:
                    assert f.kind == "where" and inc.kind == "include" and not f.exclude
                    assert f.rows() == m == inc.rows()
                    for route in ("list", "mask", "auto"):
                        idx.set_where_route(route)
                        for metric, k in check_search(idx, f, inc if route == "list" else None, ref, ids[keep], q, m, (dim, n, clause, mode, route)):
                            lw, scan = idx.last_where(), idx.last_scan()["variant"]
                            assert lw["m"] == m
                            if route == "list":
                                assert lw["route"] == 0
                                if m:
                                    assert not masked(scan), (dim, n, clause, metric, k, scan)
                            elif route == "mask":
                                ladder = bool(m) and min(k, m) <= KFAST_MAX and special
                                assert lw["route"] == (1 if ladder else 0), (dim, n, clause, metric, k, lw)
                                if ladder:
                                    assert masked(scan), (dim, n, clause, metric, k, scan)
                                    masked_seen["mask"] += 1
                    idx.set_where_route("auto")
    assert (masked_seen["mask"] > 0) == special


def test_auto_takes_the_list_at_ten_per_cent_and_the_ladder_at_fifty(V, O, no_floors):
    """int8 first: the ladder streams len * ldb bytes, the list m * ld * 4 -- the crossover is at a quarter of the rows."""
    rng = np.random.default_rng(41)
    n, dim = 20_000, 384
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    idx.set_single_filter("i8")
    q = rng.standard_normal(dim)
    values = rng.permutation(n).astype(np.int64)
    with idx.make_attribute(ids, values) as col:
        for share, route in ((0.10, 0), (0.50, 1)):
            hi = int(n * share) - 1
            keep = values <= hi
            ref = O.FlatOracle(dim, ids[keep], rows[keep])
            ri, rs = ref.search(q, 10, COS)
            with idx.make_filter_where([(col, 0, hi)]) as f:
                gi, gs = idx.search_arrays(q, 10, COS, filter=f)
                assert gi.tolist() == ri.tolist() and bits(gs) == bits(rs)
                lw = idx.last_where()
                assert lw["route"] == route and lw["m"] == int(keep.sum()), (share, lw)
                assert masked(idx.last_scan()["variant"]) == bool(route)
                if route:
                    assert family(idx.last_scan()["variant"]) == "i8"
        # f32 first: the list whatever is kept
        idx.set_single_filter("f32")
        with idx.make_filter_where([(col, None, None)]) as f:
            idx.search_arrays(q, 10, COS, filter=f)
            assert idx.last_where()["route"] == 0 and not masked(idx.last_scan()["variant"])


def test_clauses_are_anded_signed_and_blind_to_rows_without_a_value(V, O):
    rng = np.random.default_rng(43)
    n, dim = 4133, 50
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    q = rng.standard_normal(dim)
    cols, model = [], []
    for c in range(3):
        has = rng.random(n) < 0.8
        values = rng.integers(-50, 50, size=n).astype(np.int64)
        values[rng.random(n) < 0.01] = I64_MIN
        values[rng.random(n) < 0.01] = I64_MAX
        cols.append(idx.make_attribute(ids[has], values[has]))
        model.append((has, values))
    cases = [
        [(0, -10, 10), (1, 0, None)],
        [(0, -10, 10), (0, -3, 3, True)],                      # one column twice
        [(0, None, -1), (1, None, -1), (2, None, -1)],          # signed: INT64_MIN passes, INT64_MAX does not
        [(0, None, None), (1, None, None), (2, None, None), (0, 1, 0, True)],  # four clauses: the rows with all three values
        [(2, I64_MAX, I64_MAX)], [(2, I64_MIN, I64_MIN, True)],
    ]
    for case in cases:
        keep = np.ones(n, bool)
        for cl in case:
            keep &= passes(*model[cl[0]], *cl[1:])
        m = int(keep.sum())
        assert 0 < m < n
        ref = O.FlatOracle(dim, ids[keep], rows[keep])
        with idx.make_filter_where([(cols[cl[0]],) + tuple(cl[1:]) for cl in case]) as f:
            assert f.rows() == m
            for metric in (COS, MAN):
                ri, rs = ref.search(q, 20, metric)
                gi, gs = idx.search_arrays(q, 20, metric, filter=f)
                assert gi.tolist() == ri.tolist() and bits(gs) == bits(rs), case
    for c in cols:
        c.close()


# ---- 2. staleness ------------------------------------------------------------------------------------
def test_token_follows_the_rows_and_the_column(V, O):
    rng = np.random.default_rng(47)
    n, dim = 4133, 384
    ids = np.arange(n, dtype=np.uint64) * np.uint64(2)
    rows = rng.standard_normal((n, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    q = rng.standard_normal(dim)
    held = {int(i): int(v) for i, v in zip(ids[::2], rng.integers(-100, 100, size=ids[::2].size))}
    held[20_001] = 5  # an id the index does not hold yet
    col = idx.make_attribute(list(held), list(held.values()))
    f = idx.make_filter_where([(col, 0, 50)])

    def agree(resolves):
        before = idx.last_where()
        eids, evals = idx.export()
        keep = np.array([0 <= held.get(int(i), -1) <= 50 for i in eids])
        assert col.rows() == sum(int(i) in held for i in eids)
        ref = O.FlatOracle(dim, eids[keep], evals[keep])
        with idx.make_filter_where([(col, 0, 50)]) as fresh:
            for route in ("list", "mask"):
                idx.set_where_route(route)
                for metric in (COS, MAN):
                    for k in (10, 61):
                        ri, rs = ref.search(q, k, metric)
                        gi, gs = idx.search_arrays(q, k, metric, filter=f)
                        fi, fs = idx.search_arrays(q, k, metric, filter=fresh)
                        assert gi.tolist() == ri.tolist() and bits(gs) == bits(rs)
                        assert fi.tolist() == ri.tolist() and bits(fs) == bits(rs)
            assert f.rows() == fresh.rows() == int(keep.sum())
        after = idx.last_where()
        # the old token and the fresh one were each resolved once, the column once at most (whoever came first)
        assert after["resolutions"] - before["resolutions"] == (2 if resolves else 1), (before, after)
        assert after["column_resolutions"] - before["column_resolutions"] == (1 if resolves else 0), (before, after)

    agree(False)
    idx.add(V.Vector(id=20_001, values=list(q * 1.5)))  # the waiting id arrives with its value: the best row
    agree(True)
    assert idx.search_arrays(q, 1, COS, filter=f)[0].tolist() == [20_001]
    idx.add_rows(np.array([20_005, 20_007], dtype=np.uint64), np.stack([q * 1.25, rng.standard_normal(dim)]))
    agree(True)
    idx.delete(int(ids[0]))
    agree(True)
    idx.delete_many([int(x) for x in ids[10:400]])
    agree(True)
    idx.update_rows(ids[500:510], rng.standard_normal((10, dim)))  # in place: nothing to resolve, the answers follow the values
    agree(False)
    idx.update_rows(np.array([30_001], dtype=np.uint64), (q * 2.0)[None, :], insert_missing=True)  # appends: a mutation
    agree(True)
    # AttrColumn.set: a value moves across a bound, a row that had none gets one, an id added later gets one
    inside = next(i for i in ids[400:].tolist() if 0 <= held.get(i, -1) <= 50)
    without = next(i for i in ids[401::2].tolist() if i not in held)
    for upd in ({inside: 51}, {without: 0}, {20_005: 50, 30_001: 1, 40_001: 7}):
        held.update(upd)
        col.set(list(upd), list(upd.values()))
        agree(True)
    assert idx.search_arrays(q, 1, DOT, filter=f)[0].tolist() == [30_001]  # 2 q: the largest dot product, kept since the set
    # a refused set changes nothing and makes nothing stale
    with pytest.raises(V.IndexOpError, match="id 7 is given two different values"):
        col.set([9, 7, 9, 7], [1, 2, 3, 4])
    agree(False)
    f.close()
    col.close()


# ---- 3. lifetime and refusals ------------------------------------------------------------------------
def test_lifetime_and_refusals(V, O):
    rng = np.random.default_rng(53)
    n, dim = 500, 384
    ids = np.arange(n, dtype=np.uint64)
    rows = rng.standard_normal((n, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    q = rng.standard_normal(dim)
    col = idx.make_attribute(ids, np.arange(n, dtype=np.int64))
    g = idx.make_filter([1, 2, 3])
    assert col.token != 0 and g.token not in (0, col.token)  # one token space
    f = idx.make_filter_where([(col, 100, 199)])
    assert f.token not in (0, col.token, g.token) and f.rows() == 100
    ref = O.FlatOracle(dim, ids[100:200], rows[100:200])
    ri, rs = ref.search(q, 10, COS)
    # a column closed while a token lives: the token keeps working, also through a re-resolution
    tok = col.token
    col.close()
    with pytest.raises(V.IndexOpError, match="closed"):
        col.rows()
    out = C.c_uint64(0)
    assert idx._L.vl_index_attr_rows(idx._h, tok, C.byref(out)) == VL_ERR_INVALID_ARG
    assert "attribute column" in V._last_error()
    gi, gs = idx.search_arrays(q, 10, COS, filter=f)
    assert gi.tolist() == ri.tolist() and bits(gs) == bits(rs)
    idx.delete(499)
    gi, gs = idx.search_arrays(q, 10, COS, filter=f)
    assert gi.tolist() == ri.tolist() and bits(gs) == bits(rs) and f.rows() == 100
    with pytest.raises(V.IndexOpError, match="attribute column"):
        idx.make_filter_where([(tok, 0, 1)])  # the destroyed column is unknown to new tokens
    # a closed token
    out_ids, out_scores, out_n = np.zeros(10, np.uint64), np.zeros(10), C.c_uint64(0)
    raw = lambda index, t: index._L.vl_index_search_filtered(index._h, t, q.ctypes.data, q.size, 10, COS, 10, out_ids.ctypes.data,
                                                             out_scores.ctypes.data, C.byref(out_n))
    assert raw(idx, f.token) == 0 and out_n.value == 10
    twin = idx.clone()
    assert raw(twin, f.token) == VL_ERR_INVALID_ARG  # a clone does not copy tokens
    ftok = f.token
    f.close()
    assert raw(idx, ftok) == VL_ERR_INVALID_ARG
    with pytest.raises(V.IndexOpError, match="closed"):
        f.rows()
    # clause counts, reserved, negate, an unknown column
    col = idx.make_attribute([1, 2], [10, 20])
    with pytest.raises(V.IndexOpError, match="1 to 4 clauses"):
        idx.make_filter_where([])
    with pytest.raises(V.IndexOpError, match="1 to 4 clauses"):
        idx.make_filter_where([(col, 0, 1)] * 5)
    from vectorlite_amd import _make_filter_where
    with pytest.raises(V.IndexOpError, match="reserved"):
        _make_filter_where(idx._L, idx._h, idx, [(col, 0, 1)], reserved=1)
    with pytest.raises(V.IndexOpError, match="negate"):
        idx.make_filter_where([(col, 0, 1, 2)])
    with pytest.raises(V.IndexOpError, match="attribute column"):
        idx.make_filter_where([(g.token, 0, 1)])  # a filter token is no column
    with pytest.raises(V.IndexOpError, match="attribute column"):
        idx.make_filter_where([(0, 0, 1)])
    with pytest.raises(V.IndexOpError, match="id 6 is given two different values"):
        idx.make_attribute([9, 6, 5, 9, 6, 5], [1, 2, 3, 4, 5, 3])
    with idx.make_attribute([5, 5, 6], [1, 1, 2]) as same:  # exact repeats are fine
        assert same.rows() == 2
    with pytest.raises(ValueError):
        idx.search_arrays(q, 10, COS, exclude=idx.make_filter_where([(col, 0, 100)]))  # a predicate token is no exclusion
    # errors are the include token's
    with idx.make_filter_where([(col, 0, 100)]) as h:
        with pytest.raises(V.DimensionMismatch):
            idx.search_arrays(q[:-1], 10, COS, filter=h)
        with pytest.raises((V.IndexOpError, V.VectorLiteError)):
            idx.search_arrays(q, 10, 9, filter=h)
        assert idx.search_arrays(q, 0, COS, filter=h)[0].size == 0
    # handles that do not serve it
    hn = V.HNSWIndex(dim, COS)
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        hn.make_attribute([1], [1])
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        hn.make_filter_where([(1, 0, 1)])
    multi = V.MultiFlatIndex(dim, devices=[0])
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        multi.make_attribute([1], [1])
    with pytest.raises(V.IndexOpError, match="single-GPU flat"):
        multi.make_filter_where([(1, 0, 1)])
    with pytest.raises(V.IndexOpError):
        multi.set_where_route("list")


# ---- 4. the consumers --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def consumer_case(V, O):
    rng = np.random.default_rng(59)
    n, dim = 20_000, 384
    ids = random_ids(rng, n)
    centres = rng.standard_normal((40, dim))
    rows = centres[rng.integers(40, size=n)] + 0.3 * rng.standard_normal((n, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    has = (np.arange(n) % 5) != 1
    values = rng.integers(0, 1000, size=n).astype(np.int64)
    col = idx.make_attribute(ids[has], values[has])
    keep = passes(has, values, 100, 699)
    where = idx.make_filter_where([(col, 100, 699)])
    include = idx.make_filter(ids[keep])
    assert where.rows() == include.rows() == int(keep.sum())
    return {"idx": idx, "ids": ids, "rows": rows, "keep": keep, "where": where, "include": include, "rng": rng, "dim": dim,
            "m": int(keep.sum()), "col": col, "has": has, "values": values}


@pytest.mark.parametrize("masked_batch", ["on", "off"])
def test_search_batch_mixes_all_three_kinds_of_token(V, O, consumer_case, masked_batch):
    c = consumer_case
    idx, ids, rng = c["idx"], c["ids"], c["rng"]
    Q = rng.standard_normal((9, c["dim"]))
    small = idx.make_filter_where([(c["col"], 5, 5)])  # a few rows: k > m for some k
    exclude = idx.make_filter(ids[::3], exclude=True)
    filters = [c["where"], c["include"], exclude, small, c["where"], exclude, c["where"], c["include"], small]
    idx.set_masked_batch(masked_batch)
    try:
        for metric, k in ((COS, 10), (DOT, 61), (MAN, 10)):
            gi, gs, gn = idx.search_batch(Q, k, metric, filters=filters)
            routed = idx.last_masked_batch()["routed"]
            for j, f in enumerate(filters):
                si, ss = idx.search_arrays(Q[j], k, metric, filter=f)
                assert gn[j] == si.size and gi[j, :si.size].tolist() == si.tolist() and bits(gs[j, :si.size]) == bits(ss), (metric, k, j)
            if masked_batch == "off":
                assert routed == 0
            elif metric != MAN and k <= KFAST_MAX:
                assert routed == sum(f.kind != "include" for f in filters)  # predicate tokens go where exclusion tokens go
        gi, gs, gn = idx.search_batch(Q, 10, COS, filter=c["where"])  # one predicate token for the batch
        ii, isc, inn = idx.search_batch(Q, 10, COS, filter=c["include"])
        assert gn.tolist() == inn.tolist() and gi.tolist() == ii.tolist() and bits(gs) == bits(isc)
    finally:
        idx.set_masked_batch("auto")
        small.close()
        exclude.close()


def test_range_mmr_and_grouped_equal_the_include_token(V, O, consumer_case):
    c = consumer_case
    idx, ids, rows, rng = c["idx"], c["ids"], c["rows"], c["rng"]
    Q = rows[[77, 1234, 9000]] + 0.02 * rng.standard_normal((3, c["dim"]))
    # a fresh token for each consumer: each one meets a token whose list is not built yet
    fresh = lambda: idx.make_filter_where([(c["col"], 100, 699)])
    inc = c["include"]
    ref = O.FlatOracle(c["dim"], ids[c["keep"]], rows[c["keep"]])
    ri, rs = ref.search(Q[0], c["m"], COS)
    t = float(rs[25])
    with fresh() as f:
        gi, gs, total = idx.search_range_arrays(Q[0], t, COS, filter=f)
        assert total == int((rs >= t).sum()) and gi.tolist() == ri[:total].tolist() and bits(gs) == bits(rs[:total])
        ii, isc, itotal = idx.search_range_arrays(Q[0], t, COS, filter=inc)
        assert (itotal, ii.tolist(), bits(isc)) == (total, gi.tolist(), bits(gs))
    with fresh() as f:
        a = idx.search_range_batch_arrays(Q, [t, 0.5, 0.2], COS, filter=f)
        b = idx.search_range_batch_arrays(Q, [t, 0.5, 0.2], COS, filter=inc)
        assert list(a[2]) == list(b[2]) and a[2][0] == int((rs >= t).sum())
        for j in range(3):
            assert a[0][j].tolist() == b[0][j].tolist() and bits(a[1][j]) == bits(b[1][j]), j
    with fresh() as f:
        for fetch_k in (20, 100):
            a = idx.search_mmr_arrays(Q[0], 8, fetch_k, 0.5, COS, filter=f)
            b = idx.search_mmr_arrays(Q[0], 8, fetch_k, 0.5, COS, filter=inc)
            assert a[0].size == 8 and a[0].tolist() == b[0].tolist() and bits(a[1]) == bits(b[1]), fetch_k
            assert np.isin(a[0], ids[c["keep"]]).all()
    with fresh() as f:
        a = idx.search_mmr_batch_arrays(Q, 8, 30, 0.5, COS, filter=f)
        b = idx.search_mmr_batch_arrays(Q, 8, 30, 0.5, COS, filter=inc)
        assert a[2].tolist() == b[2].tolist() == [8, 8, 8] and a[0].tolist() == b[0].tolist() and bits(a[1]) == bits(b[1])
    gkeys = (np.arange(ids.size, dtype=np.uint64) % np.uint64(300)) * np.uint64(0x9E3779B97F4A7C15)
    table = idx.make_groups(ids, gkeys)
    with fresh() as f:
        a = idx.search_grouped_arrays(Q[1], 10, COS, groups=table, filter=f)
        b = idx.search_grouped_arrays(Q[1], 10, COS, groups=table, filter=inc)
        assert a[0].size == 10 and all(x.tolist() == y.tolist() for x, y in zip(a[:2], b[:2])) and bits(a[2]) == bits(b[2])
        assert np.isin(a[1], ids[c["keep"]]).all()
    for mode in ("on", "off"):
        idx.set_grouped_batch(mode)
        with fresh() as f:
            a = idx.search_grouped_batch_arrays(Q, 10, COS, groups=table, filter=f)
            b = idx.search_grouped_batch_arrays(Q, 10, COS, groups=table, filter=inc)
            assert a[3].tolist() == b[3].tolist() == [10, 10, 10]
            assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and bits(a[2]) == bits(b[2]), mode
    idx.set_grouped_batch("auto")
    table.close()


# ---- 5. concurrency ------------------------------------------------------------------------------------
def test_four_threads_search_while_a_fifth_sets_the_column(V, O, consumer_case):
    c = consumer_case
    idx, ids, rows, rng = c["idx"], c["ids"], c["rows"], c["rng"]
    Q = rng.standard_normal((4, c["dim"]))
    has = c["has"]
    values = {0: c["values"].copy(), 1: c["values"].copy()}
    flip = np.nonzero(has)[0][::2]
    values[1][flip] = 999 - values[1][flip]  # state 1: half of the valued rows mirrored across the range
    col = idx.make_attribute(ids[has], values[0][has])
    want = {}
    for s in (0, 1):
        keep = passes(has, values[s], 100, 399)
        ref = O.FlatOracle(c["dim"], ids[keep], rows[keep])
        want[s] = [tuple(x.tolist() if i == 0 else bits(x) for i, x in enumerate(ref.search(q, k, COS))) for q in Q for k in (10, 61)]
    assert want[0] != want[1]
    errors, stop = [], threading.Event()
    with idx.make_filter_where([(col, 100, 399)]) as f:

        def searcher():
            try:
                while not stop.is_set():
                    for j, (q, k) in enumerate((q, k) for q in Q for k in (10, 61)):
                        gi, gs = idx.search_arrays(q, k, COS, filter=f)
                        got = (gi.tolist(), bits(gs))
                        assert got == want[0][j] or got == want[1][j], j
            except Exception as e:  # noqa: BLE001 (reported on the main thread)
                errors.append(e)
                stop.set()

        def setter():
            try:
                for step in range(12):
                    s = (step + 1) % 2
                    col.set(ids[flip], values[s][flip])
            except Exception as e:  # noqa: BLE001
                errors.append(e)
            finally:
                stop.set()

        threads = [threading.Thread(target=searcher) for _ in range(4)] + [threading.Thread(target=setter)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        # the column ends in state 0 (12 sets: 1, 0, ..., 0)
        assert [(idx.search_arrays(q, k, COS, filter=f)[0].tolist()) for q in Q for k in (10, 61)] == [w[0] for w in want[0]]
    col.close()
