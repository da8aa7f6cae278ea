"""In-place row update and upsert on flat indexes (vl_index_update, vl_index_update_bulk) through the
public interface: after update_rows the index answers every entry point as a FlatIndex built fresh from the final rows does
and as the oracle does on those rows -- ids equal, f64 scores equal bit for bit -- with tokens made before the update still
resolved, on rows whose derived copies (f32 slab, both bf16 copies, the int8 copy) had been built BEFORE the update."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, EUC, MAN, DOT = 0, 1, 2, 3
PATH_FAST = 1
SCAN16_VARIANT_BASE, SCAN8_VARIANT_BASE, SUBSET_VARIANT_BASE = 1_000_000, 2_000_000, 3_000_000
N = 8_300  # the smallest round size above the 8192 rows from which search_batch takes the MFMA filter
K = 10
STAGE_METRICS = {"i8": (COS, DOT), "bf16": (COS, EUC, DOT), "f32": (COS, EUC, MAN, DOT)}


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


def make_ids(rng, n):
    base = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(rng.integers(1 << 20))) % np.uint64(1 << 40)
    return rng.permutation(base)


def boundary_positions(n):
    """0, 15, 16, 31, 32, 63, 64, the last row, and the last row of the last whole-or-partial 16-row group before it"""
    return [0, 15, 16, 31, 32, 63, 64, n - 1, (n - 1) // 16 * 16 - 1]


def build_copies(idx, rng, dim):
    """Searches that make the index build every lazy copy it has for this dimension, so that an update must rewrite them."""
    q = rng.standard_normal(dim)
    for mode in ("i8", "bf16", "f32"):
        idx.set_single_filter(mode)
        idx.search_arrays(q, K, COS)
    idx.set_single_filter("auto")
    idx.search_batch(rng.standard_normal((8, dim)), K, COS)


def stage_of(variant):
    v = abs(variant)
    return "i8" if SCAN8_VARIANT_BASE < v < SUBSET_VARIANT_BASE else "bf16" if SCAN16_VARIANT_BASE < v < SCAN8_VARIANT_BASE else "f32"


def same_answer(got, want, ctx):
    (gi, gs), (wi, ws) = got, want
    assert np.asarray(gi).tolist() == np.asarray(wi).tolist(), ctx
    assert bits(gs) == bits(ws), ctx


def range_from_oracle(ref, n, q, min_score, metric):
    ri, rs = ref.search(q, n, metric)
    m = 0
    while m < len(rs) and rs[m] >= min_score:
        m += 1
    return ri[:m], rs[:m]


# ---- 1. equality with a fresh index and with the oracle -----------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 384])
def test_updated_index_equals_a_fresh_index_and_the_oracle(V, O, dim):
    rng = np.random.default_rng(7 + dim)
    ids, rows = make_ids(rng, N), rng.standard_normal((N, dim))
    a = V.FlatIndex(dim)
    a.add_rows(ids, rows, validate=False)
    some = rng.choice(ids, size=N // 3, replace=False)
    gone = rng.choice(ids, size=N // 50, replace=False)
    group_keys = (ids % np.uint64(97)).astype(np.uint64)
    inc, exc, groups = a.make_filter(some), a.make_filter(gone, exclude=True), a.make_groups(ids, group_keys)
    rows_before = (inc.rows(), exc.rows(), groups.rows())
    build_copies(a, rng, dim)

    others = [int(p) for p in rng.permutation(N) if int(p) not in boundary_positions(N)]
    pos = np.array(sorted(boundary_positions(N) + others[:200 - len(boundary_positions(N))]), dtype=np.int64)
    assert pos.size == 200
    new = rng.standard_normal((pos.size, dim)) * rng.choice([0.25, 1.0, 4.0], size=(pos.size, 1))
    order = rng.permutation(pos.size)  # the list is not in position order
    assert a.update_rows(ids[pos][order], new[order]) == (pos.size, 0)
    st = a.last_update()
    assert st["updated"] == pos.size and st["inserted"] == 0 and st["chunks"] == 1, st
    assert st["int8_rows"] == pos.size and st["bf16_rows"] + st["bf16_frag_rows"] >= pos.size, st  # the copies existed

    final = rows.copy()
    final[pos] = new
    assert (inc.rows(), exc.rows(), groups.rows()) == rows_before
    ei, ev = a.export()
    assert ei.tolist() == ids.tolist() and bits(ev) == bits(final)
    for p in boundary_positions(N):
        assert bits(a.get_vector(int(ids[p])).values) == bits(final[p])

    b = V.FlatIndex(dim)
    b.add_rows(ids, final, validate=False)
    ref = O.FlatOracle(dim, ids, final)
    ref_inc = O.FlatOracle(dim, ids[np.isin(ids, some)], final[np.isin(ids, some)])
    ref_exc = O.FlatOracle(dim, ids[~np.isin(ids, gone)], final[~np.isin(ids, gone)])
    b_groups = b.make_groups(ids, group_keys)
    # queries near updated rows (their new values must win) and anywhere
    Q = np.concatenate([new[:3] + 0.05 * rng.standard_normal((3, dim)), rng.standard_normal((3, dim))])
    for metric in (COS, EUC, MAN, DOT):
        for mode in ("i8", "bf16", "f32", "auto"):
            if mode in STAGE_METRICS and metric not in STAGE_METRICS[mode]:
                continue
            a.set_single_filter(mode)
            b.set_single_filter(mode)
            for qi, q in enumerate(Q):
                want = ref.search(q, K, metric)
                same_answer(a.search_arrays(q, K, metric), want, (dim, metric, mode, qi, "oracle"))
                same_answer(b.search_arrays(q, K, metric), want, (dim, metric, mode, qi, "fresh index"))
        a.set_single_filter("auto")
        b.set_single_filter("auto")
        gi, gs, gn = a.search_batch(Q, K, metric)
        for qi, q in enumerate(Q):
            wi, ws = ref.search(q, K, metric)
            assert int(gn[qi]) == K and gi[qi].tolist() == wi.tolist() and bits(gs[qi]) == bits(ws), (dim, metric, qi, "batch")
        for qi, q in enumerate(Q[:4]):
            same_answer(a.search_arrays(q, K, metric, filter=inc), ref_inc.search(q, K, metric), (dim, metric, qi, "include token"))
            same_answer(a.search_arrays(q, K, metric, exclude=exc), ref_exc.search(q, K, metric), (dim, metric, qi, "exclusion token"))
            s10 = ref.search(q, 30, metric)[1]
            thr = float(s10[29])
            ri, rs, total = a.search_range_arrays(q, thr, metric)
            wi, ws = range_from_oracle(ref, N, q, thr, metric)
            assert total == len(wi) and ri.tolist() == wi.tolist() and bits(rs) == bits(ws), (dim, metric, qi, "range")
            same_answer(a.search_mmr_arrays(q, K, 30, 0.5, metric), b.search_mmr_arrays(q, K, 30, 0.5, metric), (dim, metric, qi, "mmr"))
            ga, gb = a.search_grouped_arrays(q, K, metric, groups=groups), b.search_grouped_arrays(q, K, metric, groups=b_groups)
            assert ga[0].tolist() == gb[0].tolist() and ga[1].tolist() == gb[1].tolist() and bits(ga[2]) == bits(gb[2]), (dim, metric, qi, "grouped")
        thr = [float(ref.search(q, 20, metric)[1][19]) for q in Q]
        il, sl, totals = a.search_range_batch_arrays(Q, thr, metric)
        for qi, q in enumerate(Q):
            wi, ws = range_from_oracle(ref, N, q, thr[qi], metric)
            assert int(totals[qi]) == len(wi) and il[qi].tolist() == wi.tolist() and bits(sl[qi]) == bits(ws), (dim, metric, qi, "range batch")


# ---- 2. planted winners: the test a stale copy cannot pass --------------------------------------------------------------
def test_planted_winners_reach_rank_one_on_every_stage_and_the_old_winner_vanishes(V, O):
    """Per (stage, metric) and query: the row at a boundary position is updated to the query's own direction (cosine 1; a dot
    product of 3 |q|^2 = 192 +- 50 against gaussian rows' N(0, |q|^2), whose largest of 8300 stays below 4.5 |q| = 36 +- 5: a gap above 50;
    Euclidean distance 0) and must be rank 1; the former rank-1 row is sent to -10 q and must leave the top k.  The oracle on
    the final rows shows the gap (asserted below); a stage whose copy of either row were stale would rank them by their
    old values."""
    dim = 64
    rng = np.random.default_rng(99)
    ids, rows = make_ids(rng, N), rng.standard_normal((N, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    build_copies(idx, rng, dim)
    cur = rows.copy()
    plant_at = boundary_positions(N) + [100, 1000, 4097]
    step = 0
    for stage, metrics in STAGE_METRICS.items():
        idx.set_single_filter(stage)
        for metric in metrics:
            by_stage = 0
            for t in range(3):
                q = rng.standard_normal(dim)
                ref0 = O.FlatOracle(dim, ids, cur)
                old_winner = int(np.nonzero(ids == ref0.search(q, 1, metric)[0][0])[0][0])
                p = plant_at[step % len(plant_at)]
                step += 1
                if p == old_winner:
                    p = (p + 17) % N
                planted = q.copy() if metric in (EUC, MAN) else 3.0 * q
                assert idx.update_rows([ids[p], ids[old_winner]], np.stack([planted, -10.0 * q])) == (2, 0)
                cur[p], cur[old_winner] = planted, -10.0 * q
                wi, ws = O.FlatOracle(dim, ids, cur).search(q, K, metric)
                assert wi[0] == ids[p] and ids[old_winner] not in wi.tolist()  # the plant is what the reference says it is
                assert ws[0] - ws[1] > (0.3 if metric == COS else 50.0 if metric == DOT else 1e-3), (stage, metric, ws[:2])
                gi, gs = idx.search_arrays(q, K, metric)
                assert gi.tolist() == wi.tolist() and bits(gs) == bits(ws), (stage, metric, t)
                if stage_of(idx.last_scan()["variant"]) == stage and V.last_path() == PATH_FAST:
                    by_stage += 1
                # back to the gaussian rows (two more updates): the next query's gap is not a matter of this one's plants
                assert idx.update_rows([ids[old_winner], ids[p]], rows[[old_winner, p]]) == (2, 0)
                cur[p], cur[old_winner] = rows[p], rows[old_winner]
            assert by_stage >= 1, f"no query of ({stage}, metric {metric}) was answered by that stage itself"
    # the batch filter (MFMA pass over the fragment-major / row-major bf16 copy)
    idx.set_single_filter("auto")
    for metric in (COS, EUC, DOT):
        Q = rng.standard_normal((8, dim))
        ref0 = O.FlatOracle(dim, ids, cur)
        used, plants = set(), {}
        for qi, q in enumerate(Q):
            old_winner = int(np.nonzero(ids == ref0.search(q, 1, metric)[0][0])[0][0])
            p = plant_at[qi]
            if p in used or old_winner in used or p == old_winner:
                continue
            used |= {p, old_winner}
            # eight plants share the index: the old winners go where they disturb no other query of the batch (a short row
            # against the query for cosine and dot, a far one for Euclid)
            planted, away = (q.copy(), -10.0 * q) if metric == EUC else (3.0 * q, -0.01 * q)
            idx.update_rows([ids[old_winner], ids[p]], np.stack([away, planted]))
            cur[p], cur[old_winner] = planted, away
            plants[qi] = (p, old_winner)
        assert len(plants) >= 4
        ref = O.FlatOracle(dim, ids, cur)
        before = idx.last_filter()
        gi, gs, gn = idx.search_batch(Q, K, metric)
        for qi, q in enumerate(Q):
            wi, ws = ref.search(q, K, metric)
            if qi in plants:
                assert wi[0] == ids[plants[qi][0]] and ids[plants[qi][1]] not in wi.tolist(), (metric, qi)
            assert gi[qi].tolist() == wi.tolist() and bits(gs[qi]) == bits(ws), (metric, qi, "batch")
        for p, w in plants.values():  # back to the gaussian rows for the next metric
            idx.update_rows([ids[p], ids[w]], rows[[p, w]])
            cur[p], cur[w] = rows[p], rows[w]
        lf = idx.last_filter()
        assert lf["ksteps"] > 0 and lf["stages"] > 0, (before, lf)  # the MFMA filter ran


# ---- 3. tokens keep their state; an upsert that appends is seen as an add ---------------------------------------------------
def test_tokens_keep_their_state_and_see_appended_rows(V, O):
    dim, n = 64, N
    rng = np.random.default_rng(5)
    ids, rows = make_ids(rng, n), rng.standard_normal((n, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    new_ids = np.array([1 << 41, (1 << 41) + 1, (1 << 41) + 2], dtype=np.uint64)
    listed = np.concatenate([ids[:500], new_ids[:2]])
    inc, exc = idx.make_filter(listed), idx.make_filter(ids[100:200], exclude=True)
    groups = idx.make_groups(np.concatenate([ids, new_ids]), np.concatenate([ids, new_ids]) % np.uint64(50))
    assert (inc.rows(), exc.rows(), groups.rows()) == (500, n - 100, n)
    q = rng.standard_normal(dim)
    idx.search_arrays(q, K, COS, filter=inc)  # resolved
    # a pure update: new values through the old tokens, the same row counts
    cur = rows.copy()
    cur[7], cur[150], cur[900] = 3.0 * q, 3.0 * q, 3.0 * q
    assert idx.update_rows(ids[[7, 150, 900]], cur[[7, 150, 900]]) == (3, 0)
    assert (inc.rows(), exc.rows(), groups.rows()) == (500, n - 100, n)
    assert idx.search_arrays(q, 1, COS, filter=inc)[0].tolist() == [int(ids[7])]  # 150 and 900: one excluded below, one not listed
    assert idx.search_arrays(q, 2, COS, exclude=exc)[0].tolist() == [int(ids[7]), int(ids[900])]
    gk, gi, _ = idx.search_grouped_arrays(q, 3, COS, groups=groups)
    assert gi.tolist()[0] == int(ids[7]) and int(gk[0]) == int(ids[7]) % 50
    same_answer(idx.search_arrays(q, K, COS, filter=inc), O.FlatOracle(dim, ids[:500], cur[:500]).search(q, K, COS), "include after update")
    # an upsert that appends: tokens see the new rows as after add
    up_rows = np.stack([2.0 * q, 2.5 * q, rng.standard_normal(dim), rng.standard_normal(dim)])
    assert idx.upsert_rows([new_ids[0], ids[3], new_ids[2], new_ids[1]], up_rows) == (1, 3)
    st = idx.last_update()
    assert (st["updated"], st["inserted"]) == (1, 3)
    assert len(idx) == n + 3 and idx.export()[0][-3:].tolist() == [int(new_ids[0]), int(new_ids[2]), int(new_ids[1])]
    assert (inc.rows(), exc.rows(), groups.rows()) == (502, n + 3 - 100, n + 3)
    all_ids = np.concatenate([ids, new_ids[[0, 2, 1]]])
    cur = np.concatenate([cur, up_rows[[0, 2, 3]]])
    cur[3] = up_rows[1]
    keep = np.isin(all_ids, listed)
    same_answer(idx.search_arrays(q, K, COS, filter=inc), O.FlatOracle(dim, all_ids[keep], cur[keep]).search(q, K, COS), "include after upsert")
    same_answer(idx.search_arrays(q, K, DOT), O.FlatOracle(dim, all_ids, cur).search(q, K, DOT), "whole index after upsert")


# ---- 4. upsert: mixed present, absent and repeated ids equal the sequential loop ---------------------------------------
@pytest.mark.parametrize("stage_rows", [0, 2])
def test_upsert_equals_the_sequential_loop(V, stage_rows):
    dim, n = 100, 2_100
    rng = np.random.default_rng(11)
    ids, rows = make_ids(rng, n), rng.standard_normal((n, dim))
    ids[40], ids[1999] = ids[10], ids[10]  # three rows carry one id: only the first is rewritten
    bulk, loop = V.FlatIndex(dim), V.FlatIndex(dim)
    for idx in (bulk, loop):
        idx.add_rows(ids, rows, validate=False)
        build_copies(idx, rng, dim)
    if stage_rows:
        bulk.set_delete_bounce(48 + stage_rows * (dim * 8 + 5) + 1)  # a staging buffer of two rows
    absent = np.arange(5, dtype=np.uint64) + np.uint64(1 << 42)
    lst = np.concatenate([ids[[0, 15, 16, 10, 2099, 2095, 31]], absent[:3], ids[rng.choice(n, 30)], absent[[1, 3, 1]], ids[[15, 10]]])
    vals = rng.standard_normal((lst.size, dim))
    upd, ins = bulk.upsert_rows(lst, vals)
    seen = set(ids.tolist())
    n_upd = set()
    for i, v in zip(lst.tolist(), vals):
        if i in seen:
            loop.update(V.Vector(id=i, values=v))
            n_upd.add(i)
        else:
            loop.add(V.Vector(id=i, values=v))
            seen.add(i)
    n_ins = len(loop) - n
    assert ins == n_ins == 4 and upd == len(n_upd - set(absent.tolist())), (upd, ins)
    st = bulk.last_update()
    assert st["updated"] == upd and st["inserted"] == ins and st["chunks"] == ((upd + 1) // 2 if stage_rows else 1), st
    (bi, bv), (li, lv) = bulk.export(), loop.export()
    assert bi.tolist() == li.tolist() and bits(bv) == bits(lv)
    assert bits(bv[40]) == bits(rows[40]) and bits(bv[1999]) == bits(rows[1999]) and bits(bv[10]) == bits(vals[-1])
    for metric in (COS, EUC, MAN, DOT):
        for q in (vals[-1] + 0.01, rng.standard_normal(dim)):
            same_answer(bulk.search_arrays(q, 20, metric), loop.search_arrays(q, 20, metric), (metric, "bulk / loop"))
    assert bulk.update_rows([], np.zeros((0, dim))) == (0, 0)
    assert all(v == 0 for v in bulk.last_update().values())


# ---- 5. refusals leave export() unchanged -----------------------------------------------------------------------------------------
def test_refusals_change_nothing(V):
    dim, n = 64, 300
    rng = np.random.default_rng(3)
    ids, rows = make_ids(rng, n), rng.standard_normal((n, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)

    def unchanged(index=idx, want_ids=ids, want_rows=rows):
        ei, ev = index.export()
        assert ei.tolist() == want_ids.tolist() and bits(ev) == bits(want_rows)

    with pytest.raises(V.DimensionMismatch):
        idx.update(V.Vector(id=int(ids[0]), values=np.zeros(dim + 1)))
    with pytest.raises(ValueError):
        idx.update_rows(ids[:2], np.zeros((2, dim - 1)))
    unchanged()
    with pytest.raises(V.IndexOpError, match="Vector ID 77 does not exist"):
        idx.update(V.Vector(id=77, values=np.zeros(dim)))
    with pytest.raises(V.IndexOpError, match="Vector ID 78 does not exist"):  # the first absent id of the list, after valid ones
        idx.update_rows([ids[0], ids[1], 78, ids[2], 77], np.ones((5, dim)))
    unchanged()
    assert all(v == 0 for v in idx.last_update().values())
    hn = V.HNSWIndex(dim, V.SimilarityMetric.Cosine)
    hn.add_rows(ids[:50], rows[:50])
    for call in (lambda: hn.update(V.Vector(id=int(ids[0]), values=np.ones(dim))), lambda: hn.update_rows(ids[:2], np.ones((2, dim))),
                 lambda: hn.upsert_rows([999], np.ones((1, dim)))):
        with pytest.raises(V.IndexOpError, match="HNSW"):
            call()
    unchanged(hn, ids[:50], rows[:50])
    multi = V.MultiFlatIndex(dim, [0, 0], "replicas")
    multi.add_rows(ids, rows, validate=False)
    for call in (lambda: multi.update(V.Vector(id=int(ids[0]), values=np.ones(dim))), lambda: multi.upsert_rows(ids[:2], np.ones((2, dim)))):
        with pytest.raises(V.IndexOpError, match="multi-GPU"):
            call()
    unchanged(multi)


# ---- 6. domain changes -------------------------------------------------------------------------------------------------------------
def test_a_row_leaving_and_entering_the_fast_path_domain_switches_the_route(V, O):
    dim = 64
    rng = np.random.default_rng(21)
    ids, rows = make_ids(rng, N), rng.standard_normal((N, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    build_copies(idx, rng, dim)
    q = rng.standard_normal(dim)
    idx.search_arrays(q, K, COS)
    assert V.last_path() == PATH_FAST
    cur = rows.copy()
    for p, bad in ((16, 2.0 ** 41), (N - 1, 0.0)):  # a value beyond 2^40: out of domain; a zero row: in domain
        cur[p] = 0.0
        cur[p, 5] = bad
        idx.update_rows([ids[p]], cur[p:p + 1])
        for metric in (COS, EUC, DOT):
            same_answer(idx.search_arrays(q, K, metric), O.FlatOracle(dim, ids, cur).search(q, K, metric), (p, metric, "out"))
            if bad != 0.0:
                assert V.last_path() != PATH_FAST, (p, metric, V.last_path())
        gi, gs, _ = idx.search_batch(np.stack([q, -q]), K, COS)
        assert gi[0].tolist() == O.FlatOracle(dim, ids, cur).search(q, K, COS)[0].tolist()
        cur[p] = rows[p]
        idx.update_rows([ids[p]], cur[p:p + 1])  # and back in
        same_answer(idx.search_arrays(q, K, COS), O.FlatOracle(dim, ids, cur).search(q, K, COS), (p, "back"))
        assert V.last_path() == PATH_FAST
    ei, ev = idx.export()
    assert bits(ev) == bits(rows)


# ---- 7. searches beside a writer see whole updates only ----------------------------------------------------------------------------
def test_concurrent_searches_see_the_index_before_or_after_a_whole_update(V, O):
    dim, n_updates, n_rows_each = 64, 50, 24
    rng = np.random.default_rng(31)
    ids, rows = make_ids(rng, N), rng.standard_normal((N, dim))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    Q = rng.standard_normal((4, dim))
    target = rng.choice(N, size=n_rows_each, replace=False)
    # update v moves the 24 rows to c_v * (q_t + noise): each state has its own top k for every query
    versions = [np.stack([(1.0 + 0.01 * v) * (Q[j % 4] + 0.3 * rng.standard_normal(dim)) for j in range(n_rows_each)]) for v in range(n_updates)]
    allowed = [set() for _ in Q]
    cur = rows.copy()
    for v in range(-1, n_updates):
        if v >= 0:
            cur[target] = versions[v]
        ref = O.FlatOracle(dim, ids, cur)
        for t, q in enumerate(Q):
            wi, ws = ref.search(q, K, COS)
            allowed[t].add((tuple(wi.tolist()), tuple(bits(ws))))
    done = threading.Event()
    seen, errors = [[] for _ in Q], []

    def searcher(t):
        try:
            while True:
                last = done.is_set()
                gi, gs = idx.search_arrays(Q[t], K, COS)
                seen[t].append((tuple(gi.tolist()), tuple(bits(gs))))
                if last:
                    return
        except Exception as e:  # pragma: no cover
            errors.append(e)

    threads = [threading.Thread(target=searcher, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    try:
        for v in range(n_updates):
            assert idx.update_rows(ids[target], versions[v]) == (n_rows_each, 0)
    finally:
        done.set()
        for th in threads:
            th.join()
    assert not errors, errors
    for t in range(4):
        assert seen[t] and all(ans in allowed[t] for ans in seen[t]), t
        assert seen[t][-1] == (lambda r: (tuple(r[0].tolist()), tuple(bits(r[1]))))(O.FlatOracle(dim, ids, cur).search(Q[t], K, COS))


# ---- 8. the client layer ----------------------------------------------------------------------------------------------------------
def test_client_update_text_reembeds_in_place(V):
    from vectorlite_amd import client as VC

    class Embed:
        def dimension(self):
            return 16

        def generate_embedding(self, text):
            r = np.random.default_rng(abs(hash(text)) % (1 << 32))
            return r.standard_normal(16).tolist()

    c = VC.VectorLiteClient(Embed())
    c.create_collection("docs", VC.IndexType.Flat)
    a = c.add_text_to_collection("docs", "first text", {"v": 1})
    b = c.add_text_to_collection("docs", "second text", {"v": 1})
    c.update_text_in_collection("docs", a, "first text, corrected", {"v": 2})
    got = c.get_vector_from_collection("docs", a)
    assert got.text == "first text, corrected" and got.metadata == {"v": 2}
    assert bits(got.values) == bits(Embed().generate_embedding("first text, corrected"))
    assert c.get_collection("docs").index.export()[0].tolist() == [a, b]  # the row kept its place
    top = c.search_text_in_collection("docs", "first text, corrected", 1)
    assert top[0].id == a and top[0].text == "first text, corrected"
    with pytest.raises(VC.VectorNotFound):
        c.update_text_in_collection("docs", 12345, "nothing", None)
    c.create_collection("graph", VC.IndexType.HNSW, V.SimilarityMetric.Cosine)
    g = c.add_text_to_collection("graph", "a node", None)
    with pytest.raises(VC.VectorLiteError, match="HNSW"):
        c.update_text_in_collection("graph", g, "changed", None)
