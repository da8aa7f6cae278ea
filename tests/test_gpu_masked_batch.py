"""Batches of exclusion-filtered queries on the mask-aware MFMA pass (vl_index_set_masked_batch): row i
of search_batch(Q, k, filters=F) is what the oracle gives on the rows F[i] keeps -- ids equal, f64 scores equal bit for bit
-- in every mode, whether the pass certifies a query or hands it back; last_masked_batch() tells which it did."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, EUC, MAN, DOT = 0, 1, 2, 3
KFAST_MAX = 60
MFMA_MIN_ROWS = 8192


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


def kept_mask(ids, excluded):
    return ~np.isin(ids, np.asarray(sorted(excluded), dtype=np.uint64)) if len(excluded) else np.ones(ids.size, bool)


def exclusion_sets(rng, ids):
    """Empty, 1, 10, n / 100, n / 2, all but 70 rows, all but 3 rows, every id."""
    n = ids.size
    pick = lambda m: [int(x) for x in rng.choice(ids, size=m, replace=False)]
    return [[], pick(1), pick(10), pick(n // 100), pick(n // 2), pick(n - 70), pick(n - 3), [int(x) for x in ids]]


def oracle_rows(O, dim, ids, rows, excluded, Q, k, metric):
    """Per query (ids, score bits) of the oracle on the kept rows."""
    keep = kept_mask(ids, excluded)
    m = int(keep.sum())
    if m == 0:
        return [([], [])] * len(Q)
    ref = O.FlatOracle(dim, ids[keep], rows[keep])
    out = []
    for q in Q:
        ri, rs = ref.search(q, min(k, m), metric)
        out.append((ri.tolist(), bits(rs)))
    return out


def check_row(got, want, i, ctx):
    gi, gs, gn = got
    wi, ws = want
    assert int(gn[i]) == len(wi), (ctx, i, int(gn[i]), len(wi))
    assert gi[i, :len(wi)].tolist() == wi, (ctx, i)
    assert bits(gs[i, :len(wi)]) == ws, (ctx, i)


def build(V, rng, n, dim, scale=None):
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    if scale is not None:
        rows *= scale
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    return idx, ids, rows


# ---- 1. parity with the oracle, shared token and one token per query ---------------------------------------------
@pytest.mark.parametrize("metric", [COS, EUC, DOT])
@pytest.mark.parametrize("n,dim", [(9_000, 128), (12_345, 384), (20_000, 768)])
def test_parity_with_the_oracle_on_the_kept_rows(V, O, n, dim, metric):
    rng = np.random.default_rng(100 * dim + metric)
    idx, ids, rows = build(V, rng, n, dim)
    idx.set_masked_batch("on")
    k = 10
    sets = exclusion_sets(rng, ids)
    Q = rng.standard_normal((len(sets), dim))
    certified = 0
    # one shared token for the batch
    for excluded in sets:
        want = oracle_rows(O, dim, ids, rows, excluded, Q, k, metric)
        got = idx.search_batch(Q, k, metric, exclude=excluded)
        for i in range(len(Q)):
            check_row(got, want[i], i, (n, dim, metric, len(excluded)))
        st = idx.last_masked_batch()
        m = n - len(excluded)
        assert st["routed"] == (len(Q) if m > 0 else 0), (st, len(excluded))  # every query is eligible
        assert st["certified"] + st["redone"] == st["routed"] and st["sequences"] == (1 if m > 0 else 0), st
        assert st["lists_built"] == (1 if st["redone"] else 0), st
        certified += st["certified"]
    # one token per query: query i under set i
    filters = [idx.make_filter(s, exclude=True) for s in sets]
    try:
        got = idx.search_batch(Q, k, metric, filters=filters)
        for i, excluded in enumerate(sets):
            want = oracle_rows(O, dim, ids, rows, excluded, Q[i:i + 1], k, metric)
            check_row(got, want[0], i, (n, dim, metric, "per query", len(excluded)))
        st = idx.last_masked_batch()
        assert st["routed"] == len(sets) - 1, st  # all but the token that keeps nothing
        certified += st["certified"]
    finally:
        for f in filters:
            f.close()
    assert certified > 0, "no query was certified by the masked pass: the parity above proved nothing about it"


# ---- 2. row for row equal to the loop, handed-back queries included ------------------------------------------------
@pytest.mark.parametrize("metric", [COS, EUC, DOT])
def test_batch_rows_equal_the_single_filtered_search(V, metric):
    rng = np.random.default_rng(31 + metric)
    n, dim, k = 10_007, 384, 7
    idx, ids, rows = build(V, rng, n, dim)
    # planted exact ties at the k-th place: eight copies of one row, seven of them compete for the last places
    rows2 = rng.standard_normal((8, dim))
    rows2[:] = rows[4000]
    idx.add_rows(np.arange(8, dtype=np.uint64) + np.uint64(1 << 41), rows2, validate=False)
    idx.set_masked_batch("on")
    Q = rng.standard_normal((12, dim))
    Q[3] = 0.0                                    # a zero query
    Q[5] = rows[4000] + 1e-3 * rng.standard_normal(dim)  # next to the tied rows
    Q[7] = rng.standard_normal(dim) * 1e200       # outside the fast-path domain
    sets = [[int(x) for x in rng.choice(ids, size=s, replace=False)] for s in (0, 1, 5, 50, 500, 5000)] * 2
    filters = [idx.make_filter(s, exclude=True) for s in sets]
    try:
        gi, gs, gn = idx.search_batch(Q, k, metric, filters=filters)
        st = idx.last_masked_batch()
        fb = idx.last_filtered_batch()
        assert st["routed"] == 12 and st["redone"] >= 2, st  # the zero query and the out-of-domain one come back
        assert fb["batched"] + fb["single"] + fb["exact"] == st["redone"], (fb, st)
        for i in range(12):
            si, ss = idx.search_arrays(Q[i], k, metric, filter=filters[i])
            assert int(gn[i]) == si.size and gi[i, :si.size].tolist() == si.tolist(), (metric, i)
            assert bits(gs[i, :si.size]) == bits(ss), (metric, i)
    finally:
        for f in filters:
            f.close()


# ---- 3. mixed batches, modes, reports ---------------------------------------------------------------------------
def test_mixed_batch_and_the_three_modes(V, O):
    rng = np.random.default_rng(5)
    n, dim, k, metric = 9_500, 128, 10, COS
    idx, ids, rows = build(V, rng, n, dim)
    Q = rng.standard_normal((16, dim))
    inc_sets = [[int(x) for x in rng.choice(ids, size=300, replace=False)] for _ in range(6)]
    exc_sets = [[int(x) for x in rng.choice(ids, size=20, replace=False)] for _ in range(10)]
    filters = [idx.make_filter(s) for s in inc_sets] + [idx.make_filter(s, exclude=True) for s in exc_sets]
    want = []
    for i in range(6):
        inside = np.isin(ids, np.asarray(inc_sets[i], dtype=np.uint64))
        ri, rs = O.FlatOracle(dim, ids[inside], rows[inside]).search(Q[i], k, metric)
        want.append((ri.tolist(), bits(rs)))
    for i in range(10):
        want.append(oracle_rows(O, dim, ids, rows, exc_sets[i], Q[6 + i:7 + i], k, metric)[0])
    try:
        reports = {}
        for mode in ("on", "off", "auto"):
            idx.set_masked_batch(mode)
            got = idx.search_batch(Q, k, metric, filters=filters)
            for i in range(16):
                check_row(got, want[i], i, mode)
            reports[mode] = (idx.last_masked_batch(), idx.last_filtered_batch())
        st, fb = reports["on"]
        assert st["routed"] == 10 and st["certified"] > 0, st
        # the include jobs and what the pass handed back, nothing else
        assert fb["batched"] + fb["single"] + fb["exact"] == 6 + st["redone"], (fb, st)
        for mode in ("off", "auto"):  # today's route; on an index this small the cost rule keeps it
            st, fb = reports[mode]
            assert st["routed"] == 0 and st["sequences"] == 0, (mode, st)
            assert fb["batched"] + fb["single"] + fb["exact"] == 16, (mode, fb)
    finally:
        for f in filters:
            f.close()


def test_a_certified_batch_builds_no_position_list(V):
    rng = np.random.default_rng(6)
    n, dim = 10_000, 384
    idx, ids, rows = build(V, rng, n, dim)
    idx.set_masked_batch("on")
    Q = rng.standard_normal((8, dim))
    with idx.make_filter([int(x) for x in ids[:10]], exclude=True) as f:
        gi, gs, gn = idx.search_batch(Q, 5, COS, filter=f)
        st = idx.last_masked_batch()
        assert st == {"routed": 8, "certified": 8, "redone": 0, "sequences": 1, "lists_built": 0}, st
        # a later call that needs the list builds and uses it (a range search reads the filter's rows through it)
        ri, rs, total = idx.search_range_arrays(Q[0], -2.0, COS, filter=f, limit=20)
        assert int(total) == n - 10 and not np.isin(ri, ids[:10]).any()
        idx.set_masked_batch("off")
        oi, os_, on = idx.search_batch(Q, 5, COS, filter=f)
        assert idx.last_masked_batch()["lists_built"] == 0  # built by the range search already
        assert oi.tolist() == gi.tolist() and bits(os_) == bits(gs)


# ---- 4. staleness and concurrency -----------------------------------------------------------------------------------
def test_mutations_between_batches_and_threads(V, O):
    rng = np.random.default_rng(8)
    n, dim, k = 9_000, 128, 10
    idx, ids, rows = build(V, rng, n, dim)
    idx.set_masked_batch("on")
    Q = rng.standard_normal((6, dim))
    excluded = [int(x) for x in ids[100:130]]
    with idx.make_filter(excluded, exclude=True) as f:
        def check(ids_now, rows_now):
            want = oracle_rows(O, dim, ids_now, rows_now, excluded, Q, k, DOT)
            got = idx.search_batch(Q, k, DOT, filter=f)
            for i in range(len(Q)):
                check_row(got, want[i], i, ids_now.size)
            assert idx.last_masked_batch()["routed"] == len(Q)
            return got
        check(ids, rows)
        new_ids = np.arange(50, dtype=np.uint64) + np.uint64(1 << 42)
        new_rows = Q[np.arange(50) % 6] + 0.01 * rng.standard_normal((50, dim))  # they take over the top places
        idx.add_rows(new_ids, new_rows, validate=False)
        ids2, rows2 = np.concatenate([ids, new_ids]), np.concatenate([rows, new_rows])
        check(ids2, rows2)
        idx.delete(int(new_ids[0]))
        ids3, rows3 = np.delete(ids2, n), np.delete(rows2, n, axis=0)
        check(ids3, rows3)
        gone = np.concatenate([np.arange(200, 260), np.arange(n, n + 20)])
        idx.delete_many([int(x) for x in ids3[gone]])
        ids4, rows4 = np.delete(ids3, gone), np.delete(rows3, gone, axis=0)
        lone = check(ids4, rows4)
        results, errors = [None] * 4, []

        def worker(t):
            try:
                results[t] = idx.search_batch(Q, k, DOT, filter=f)
            except Exception as e:  # noqa: BLE001
                errors.append(e)
        threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for r in results:
            assert r[0].tolist() == lone[0].tolist() and bits(r[1]) == bits(lone[1]) and r[2].tolist() == lone[2].tolist()


# ---- 5. ineligible batches keep the old route ---------------------------------------------------------------------------
def test_ineligible_batches_stay_on_the_jobs_route(V, O):
    rng = np.random.default_rng(9)
    n, dim = 9_000, 128
    idx, ids, rows = build(V, rng, n, dim)
    idx.set_masked_batch("on")
    excluded = [int(x) for x in ids[:25]]
    Q = rng.standard_normal((5, dim))

    def unrouted(index, Qs, k, metric, excl, i_ids, i_rows):
        want = oracle_rows(O, dim, i_ids, i_rows, excl, Qs, k, metric)
        got = index.search_batch(Qs, k, metric, exclude=excl)
        for i in range(len(Qs)):
            check_row(got, want[i], i, (k, metric))
        st = index.last_masked_batch()
        assert st["routed"] == 0 and st["sequences"] == 0, st

    unrouted(idx, Q, 10, MAN, excluded, ids, rows)               # no MFMA shape for Manhattan
    unrouted(idx, Q, KFAST_MAX + 1, COS, excluded, ids, rows)    # k beyond the candidate list's margin
    unrouted(idx, Q[:1], 10, COS, excluded, ids, rows)           # a batch of one
    idx.force_path(V.PATH_EXACT_SELECT)
    unrouted(idx, Q, 10, COS, excluded, ids, rows)               # a forced path
    idx.force_path(0)
    small, s_ids, s_rows = build(V, rng, MFMA_MIN_ROWS - 1, dim)
    small.set_masked_batch("on")
    unrouted(small, Q, 10, COS, [int(x) for x in s_ids[:25]], s_ids, s_rows)  # below MFMA_MIN_ROWS
    # and the eligible call on the same handle is routed
    idx.search_batch(Q, 10, COS, exclude=excluded)
    assert idx.last_masked_batch()["routed"] == len(Q)


def test_nan_scores_fail_only_when_a_kept_row_scores_nan(V):
    rng = np.random.default_rng(10)
    n, dim = 9_000, 128
    ids = random_ids(rng, n)
    rows = rng.standard_normal((n, dim))
    rows[500, 3] = np.nan  # (a row outside the f32 domain: the handle's batches keep the jobs route)
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    idx.set_masked_batch("on")
    Q = rng.standard_normal((4, dim))
    hidden = [int(ids[500])] + [int(x) for x in ids[:9]]
    gi, gs, gn = idx.search_batch(Q, 5, COS, exclude=hidden)  # the NaN row is hidden: the call succeeds
    assert gn.tolist() == [5] * 4 and not np.isnan(gs).any()
    for i in range(4):
        si, ss = idx.search_arrays(Q[i], 5, COS, exclude=hidden)
        assert gi[i].tolist() == si.tolist() and bits(gs[i]) == bits(ss)
    with pytest.raises(V.NaNScore):
        idx.search_batch(Q, 5, COS, exclude=[int(x) for x in ids[:9]])  # it is kept: the single call's error
