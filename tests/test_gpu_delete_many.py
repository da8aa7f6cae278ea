"""delete_many(ids) (vl_index_delete_bulk) leaves an index in exactly the state `for id in ids: delete(id)` leaves it in.

Twin indexes hold the same rows; one takes delete_many, the other the loop of single deletes.  Length, exported ids and the
exported f64 bytes are compared between the twins with ==, searches in all four metrics against oracle.FlatOracle over the
surviving rows (ids and score bits ==).  N = 3000 rows; dims 3 (24-byte master rows: no 16-byte path), 100 and 384; the delete
compaction buffer set to 16 KiB (20 rows at dim 100) so that the plan of csrc/delete_plan.hpp cuts the index into many
segments of both kinds, and once left at its default."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 3000
SMALL_BOUNCE = 16 << 10
TRIPLE = np.uint64(777_000_000_007)   # one id stored three times (unvalidated add)
TRIPLE_AT = (10, 500, 2500)


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


def unit_rows(rng, n, dim):
    rows = rng.standard_normal((n, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    return np.ascontiguousarray(rows)


def make_data(dim, n=N):
    """rows, and ids permuted so that id != position, one of them three times"""
    rng = np.random.default_rng(1000 + dim)
    rows = unit_rows(rng, n, dim)
    ids = (rng.permutation(n).astype(np.uint64) * np.uint64(2654435761) + np.uint64(99)) % np.uint64(1 << 40)
    for p in TRIPLE_AT:
        ids[p] = TRIPLE
    return ids, rows, rng


def removed_sets(ids, rng):
    """name -> the list handed to delete_many / looped over (ids, in the order given)"""
    n = ids.size
    absent = np.array([5, 1 << 50, (1 << 64) - 1], dtype=np.uint64)  # none of them is stored
    sets = {
        "none": ids[:0],
        "first": ids[:1],
        "last": ids[n - 1:],
        "middle": ids[n // 2:n // 2 + 1],
        "every other": ids[::2],
        "long run": ids[n // 5:n // 5 + n // 3],
        "all": ids.copy(),
        "only absent": absent,
    }
    for pct in (1, 10, 50, 99):
        sets["random %d%%" % pct] = ids[np.sort(rng.choice(n, size=n * pct // 100, replace=False))]
    # absent ids, ids named twice and the triple id, in no order
    mixed = np.concatenate([sets["random 10%"], absent, sets["random 10%"][:40], [TRIPLE], sets["random 1%"]])
    sets["mixed, shuffled"] = rng.permutation(mixed)
    return sets


def survivors(ids, rows, gone):
    keep = ~np.isin(ids, np.asarray(gone, dtype=np.uint64))
    return ids[keep], rows[keep]


def same_state(a, b):
    assert len(a) == len(b)
    (ia, va), (ib, vb) = a.export(), b.export()
    assert ia.tolist() == ib.tolist()
    assert va.tobytes() == vb.tobytes()


def searches_match(O, idx, dim, ids, rows, queries, k=10):
    ref = O.FlatOracle(dim, ids, rows)
    assert len(idx) == len(ref)
    for metric in range(4):
        for q in queries:
            gi, gs = idx.search_arrays(q, k, metric)
            ri, rs = ref.search(q, k, metric)
            assert gi.tolist() == ri.tolist(), metric
            assert bits(gs) == bits(rs), metric


def loop_delete(idx, ids):
    for i in ids.tolist():
        idx.delete(i)


@pytest.mark.parametrize("dim,bounce", [(3, SMALL_BOUNCE), (100, SMALL_BOUNCE), (384, SMALL_BOUNCE), (100, 0)])
def test_delete_many_equals_the_loop_of_deletes(V, O, dim, bounce):
    ids, rows, rng = make_data(dim)
    queries = [rows[7] + 0.05 * rng.standard_normal(dim), rng.standard_normal(dim)]
    for name, gone in removed_sets(ids, rng).items():
        bulk, loop = V.FlatIndex(dim), V.FlatIndex(dim)
        for idx in (bulk, loop):
            idx.add_rows(ids, rows, validate=False)
        if bounce:
            bulk.set_delete_bounce(bounce)
        kept_ids, kept_rows = survivors(ids, rows, gone)
        removed = bulk.delete_many(gone)
        loop_delete(loop, gone)
        assert removed == N - kept_ids.size, name
        same_state(bulk, loop)
        assert bulk.export()[0].tolist() == kept_ids.tolist(), name
        searches_match(O, bulk, dim, kept_ids, kept_rows, queries)
        # what the call did on the device
        st = bulk.last_delete()
        print(dim, bounce, name, st)
        hit = np.flatnonzero(np.isin(ids, gone))
        if hit.size == 0:
            assert st["removed"] == 0 and st["moved"] == 0, name
            continue
        assert st["removed"] == hit.size, name
        assert st["moved"] == (N - hit[0]) - hit.size, name  # rows behind the first hole minus rows removed
        assert (st["direct_launches"] + st["bounced_segments"] > 0) == (st["moved"] > 0), name
        if bounce and name == "random 50%":
            assert st["direct_launches"] > 0 and st["bounced_segments"] > 0, st
        if name == "first":  # one hole at row 0: nothing but single rows may move in place
            per_array = [-(-(N - 1) // max(1, (bounce or (64 << 20)) // p)) for p in (dim * 8, -(-dim // 4) * 16, 4, 1)]
            assert st["bounced_segments"] + st["direct_launches"] == sum(per_array), (st, per_array)


def test_growth_filters_groups_and_clones_around_a_compaction(V, O):
    dim = 100
    ids, rows, rng = make_data(dim)
    sets = removed_sets(ids, rng)
    queries = [rows[11] + 0.05 * rng.standard_normal(dim), rng.standard_normal(dim)]
    bulk, loop = V.FlatIndex(dim), V.FlatIndex(dim)
    for idx in (bulk, loop):
        idx.add_rows(ids, rows, validate=False)
    bulk.set_delete_bounce(SMALL_BOUNCE)
    # a filter and a group table made before the delete
    f_ids = ids[rng.choice(N, size=900, replace=False)]
    filt = bulk.make_filter(f_ids)
    g_ids = ids[rng.choice(N, size=1500, replace=False)]
    g_keys = (g_ids % np.uint64(37)) * np.uint64(0x9E3779B97F4A7C15)
    groups = bulk.make_groups(g_ids, g_keys)
    bulk.search_arrays(queries[0], 5, 0, filter=filt)  # both resolved against the rows as they are now
    bulk.search_grouped_arrays(queries[0], 5, 0, groups=groups)
    before = bulk.clone()

    gone = sets["mixed, shuffled"]
    bulk.delete_many(gone)
    loop_delete(loop, gone)
    same_state(bulk, loop)
    kept_ids, kept_rows = survivors(ids, rows, gone)
    searches_match(O, bulk, dim, kept_ids, kept_rows, queries)
    after = bulk.clone()
    # the filter and the group table, over the surviving subset
    in_f = np.isin(kept_ids, f_ids)
    searches_f = O.FlatOracle(dim, kept_ids[in_f], kept_rows[in_f])
    in_g = np.isin(kept_ids, g_ids)
    ranked_g = O.FlatOracle(dim, kept_ids[in_g], kept_rows[in_g])
    key_of = dict(zip(g_ids.tolist(), g_keys.tolist()))
    for metric in range(4):
        for q in queries:
            gi, gs = bulk.search_arrays(q, 10, metric, filter=filt)
            ri, rs = searches_f.search(q, 10, metric)
            assert gi.tolist() == ri.tolist() and bits(gs) == bits(rs)
            ri, rs = ranked_g.search(q, int(in_g.sum()), metric)
            want, seen = [], set()
            for i, s in zip(ri.tolist(), bits(rs)):
                if key_of[i] not in seen:
                    seen.add(key_of[i])
                    want.append((key_of[i], i, s))
                if len(want) == 8:
                    break
            gk, gi, gs = bulk.search_grouped_arrays(q, 8, metric, groups=groups)
            assert list(zip(gk.tolist(), gi.tolist(), bits(gs))) == want
    # clones: the one taken before still holds every row, the one taken after is the compacted index
    assert len(before) == N and before.export()[0].tolist() == ids.tolist()
    searches_match(O, before, dim, ids, rows, queries[:1])
    same_state(after, bulk)
    searches_match(O, after, dim, kept_ids, kept_rows, queries[:1])

    # growth after a compaction (past the capacity the arrays had), another bulk delete, another search
    more = 1700
    new_rows = unit_rows(rng, more, dim)
    new_ids = np.arange(more, dtype=np.uint64) + np.uint64(1 << 41)
    for idx in (bulk, loop):
        idx.add_rows(new_ids, new_rows, validate=True)
    all_ids, all_rows = np.concatenate([kept_ids, new_ids]), np.concatenate([kept_rows, new_rows])
    gone2 = rng.permutation(np.concatenate([all_ids[::7], new_ids[-50:], gone[:20]]))
    assert bulk.delete_many(gone2) == np.isin(all_ids, gone2).sum()
    loop_delete(loop, gone2)
    same_state(bulk, loop)
    kept2_ids, kept2_rows = survivors(all_ids, all_rows, gone2)
    searches_match(O, bulk, dim, kept2_ids, kept2_rows, queries)
    st = bulk.last_delete()
    assert st["direct_launches"] > 0 and st["bounced_segments"] > 0, st
    assert bulk.delete_many([]) == 0 and len(bulk) == kept2_ids.size


def test_hnsw_delete_many_is_the_loop_with_its_stop_at_an_absent_id(V):
    dim, n = 16, 600
    rng = np.random.default_rng(5)
    rows = unit_rows(rng, n, dim)
    ids = rng.permutation(n).astype(np.uint64) + np.uint64(1000)
    bulk, loop = V.HNSWIndex(dim, V.SimilarityMetric.Cosine), V.HNSWIndex(dim, V.SimilarityMetric.Cosine)
    for idx in (bulk, loop):
        idx.add_rows(ids, rows)
    q = rng.standard_normal(dim)

    def same():
        assert len(bulk) == len(loop)
        assert bulk.export()[0].tolist() == loop.export()[0].tolist()
        (bi, bs), (li, ls) = bulk.search_arrays(q, 10, 0), loop.search_arrays(q, 10, 0)
        assert bi.tolist() == li.tolist() and bits(bs) == bits(ls)

    first = ids[::5]
    assert bulk.delete_many(first) == first.size
    loop_delete(loop, first)
    same()
    assert len(bulk) == n - first.size
    # an absent id in the middle: the error of the loop, and the prefix stays deleted
    bad = np.concatenate([ids[1:40:5], [np.uint64(5)], ids[2:40:5]])
    with pytest.raises(V.IndexOpError, match="Vector ID 5 does not exist"):
        bulk.delete_many(bad)
    with pytest.raises(V.IndexOpError, match="Vector ID 5 does not exist"):
        loop_delete(loop, bad)
    same()
    assert len(bulk) == n - first.size - 8
    # an id named twice: the second time it does not exist any more
    twice = np.array([ids[3], ids[8], ids[3], ids[13]], dtype=np.uint64)
    with pytest.raises(V.IndexOpError, match=f"Vector ID {int(ids[3])} does not exist"):
        bulk.delete_many(twice)
    with pytest.raises(V.IndexOpError, match=f"Vector ID {int(ids[3])} does not exist"):
        loop_delete(loop, twice)
    same()
    assert bulk.delete_many([]) == 0


@pytest.mark.parametrize("mode", ["replicas", "row_shards"])
def test_multi_handle_with_one_ordinal_twice_matches_the_single_index(V, O, mode):
    dim = 100
    ids, rows, rng = make_data(dim)
    queries = [rows[3] + 0.05 * rng.standard_normal(dim), rng.standard_normal(dim)]
    multi, single = V.MultiFlatIndex(dim, [0, 0], mode), V.FlatIndex(dim)
    for a, b in ((0, 1100), (1100, N)):
        for idx in (multi, single):
            idx.add_rows(ids[a:b], rows[a:b], validate=False)
    multi.set_delete_bounce(SMALL_BOUNCE)
    gone = removed_sets(ids, rng)["mixed, shuffled"]
    kept_ids, kept_rows = survivors(ids, rows, gone)
    assert multi.delete_many(gone) == single.delete_many(gone) == N - kept_ids.size
    assert len(multi) == len(single) == kept_ids.size
    assert sum(multi.parts()["rows"]) == kept_ids.size * (2 if mode == "replicas" else 1)
    searches_match(O, multi, dim, kept_ids, kept_rows, queries)
    searches_match(O, single, dim, kept_ids, kept_rows, queries)
    for metric in (0, 1):
        (mi, ms), (si, ss) = multi.search_arrays(queries[0], 60, metric), single.search_arrays(queries[0], 60, metric)
        assert mi.tolist() == si.tolist() and bits(ms) == bits(ss)
    # rows added behind the compaction land where a single index puts them, and go again
    new_rows = unit_rows(rng, 300, dim)
    new_ids = np.arange(300, dtype=np.uint64) + np.uint64(1 << 41)
    for idx in (multi, single):
        idx.add_rows(new_ids, new_rows, validate=True)
    gone2 = np.concatenate([kept_ids[::3], new_ids[::2]])
    all_ids, all_rows = np.concatenate([kept_ids, new_ids]), np.concatenate([kept_rows, new_rows])
    kept2_ids, kept2_rows = survivors(all_ids, all_rows, gone2)
    assert multi.delete_many(gone2) == gone2.size
    searches_match(O, multi, dim, kept2_ids, kept2_rows, queries)
