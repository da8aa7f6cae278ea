"""The argument rules of the five single-query entry points of a flat index (search, search_filtered, search_range,
search_mmr, search_grouped) through the C ABI: which check answers when two arguments are wrong at once, the status and
the vl_last_error text of each refusal, and that the handle's next valid call after every refusal returns the oracle's
ids and score bits (the scratch a refused call borrowed went back usable).  Error returns only; nothing here faults."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS = 0
N, DIM, BAD_LEN, BAD_METRIC = 64, 8, 5, 9
OK, ERR_DIM_MISMATCH, ERR_NAN_SCORE, ERR_INVALID_ARG = 0, 1, 5, 8
NO_SUCH = 0xDEAD00000000          # a token no handle of this process ever receives
CAP = 16                          # slots of every output buffer
NAN_ID = 999
ENTRIES = ("search", "filtered", "range", "mmr", "grouped")

UNKNOWN_FILTER = "unknown or destroyed filter"
UNKNOWN_GROUPS = "unknown or destroyed group table"
UNKNOWN_METRIC = "unknown metric"
K_LIMIT = "grouped search: k exceeds VL_GROUPED_MAX_K (1024)"
NAN_THRESHOLD = "min_score is NaN"
NAN_SCORE = "NaN similarity score: the reference panics in partial_cmp().unwrap()"
DIM_TEXT = "Dimension mismatch: expected %d, got %d" % (DIM, BAD_LEN)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64).tolist()


class Handle:
    """One index with a filter and a group table, called through the raw C ABI with any argument overridden."""

    def __init__(self, V, ids, rows, filter_ids, group_ids, group_keys):
        self.V, self.L = V, V._lib.load()
        self.idx = V.FlatIndex(DIM)
        if len(ids):
            self.idx.add_rows(ids, rows, validate=False)
        self.filt = self.idx.make_filter(filter_ids)
        self.table = self.idx.make_groups(group_ids, group_keys)
        self.keys = np.zeros(CAP, dtype=np.uint64)
        self.ids = np.zeros(CAP, dtype=np.uint64)
        self.scores = np.zeros(CAP, dtype=np.float64)

    def call(self, entry, q, q_len=DIM, metric=COS, token=None, groups=None, k=5, min_score=0.0, fetch_k=10, lam=0.5):
        """-> (status, n, total or None)"""
        L, h = self.L, self.idx._h
        q = np.ascontiguousarray(q, dtype=np.float64)
        n, total = C.c_uint64(77), C.c_uint64(77)
        token = self.filt.token if token is None else token
        groups = self.table.token if groups is None else groups
        pi, ps, pk = self.ids.ctypes.data, self.scores.ctypes.data, self.keys.ctypes.data
        if entry == "search":
            rc = L.vl_index_search(h, q.ctypes.data_as(C.POINTER(C.c_double)), q_len, k, metric,
                                   self.ids.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   self.scores.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n))
        elif entry == "filtered":
            rc = L.vl_index_search_filtered(h, token, q.ctypes.data, q_len, k, metric, CAP, pi, ps, C.addressof(n))
        elif entry == "range":
            rc = L.vl_index_search_range(h, token, q.ctypes.data, q_len, min_score, metric, pi, ps, CAP, C.byref(n), C.byref(total))
            return rc, n.value, total.value
        elif entry == "mmr":
            rc = L.vl_index_search_mmr(h, token, q.ctypes.data, q_len, k, fetch_k, lam, metric, CAP, pi, ps, C.byref(n))
        else:
            rc = L.vl_index_search_grouped(h, groups, token, q.ctypes.data, q_len, k, metric, CAP, pk, pi, ps, C.byref(n))
        return rc, n.value, None

    def error(self):
        return self.V._last_error()

    def dim_pair(self):
        e, a = C.c_uint64(0), C.c_uint64(0)
        self.L.vl_last_dim_mismatch(C.byref(e), C.byref(a))
        return e.value, a.value


@pytest.fixture(scope="module")
def world():
    """The rows, the valid call of every entry point and the oracle's answer to it (computed once, never changed)."""
    import vectorlite_amd as V
    from oracle import oracle as O
    n_dev, _ = V.runtime_info()
    assert n_dev > 0, "GPU tests need a HIP device"
    rng = np.random.default_rng(64008)
    ids = (np.arange(N, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 40)
    rows = rng.standard_normal((N, DIM))
    q = rng.standard_normal(DIM)
    in_filter = np.zeros(N, dtype=bool)
    in_filter[rng.permutation(N)[:16]] = True
    gkeys = (np.arange(N, dtype=np.uint64) % np.uint64(8)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(3)
    expect = {"search": O.FlatOracle(DIM, ids, rows).search(q, 5, COS)}
    # every other entry point is given the filter: the FlatIndex of its 16 rows in storage order, ranked once
    fi, fs = O.FlatOracle(DIM, ids[in_filter], rows[in_filter]).search(q, 16, COS)
    expect["filtered"] = (fi[:5], fs[:5])
    min_score = float(fs[6])
    m = int((fs >= min_score).sum())
    expect["range"] = (fi[:m], fs[:m])
    # MMR over the best 10: sel[0] = the best, then the largest lam * score - (1 - lam) * max similarity to a chosen one
    pos_of = {int(i): p for p, i in enumerate(ids.tolist())}
    ci, cs = fi[:10], fs[:10]
    cand = [rows[pos_of[int(i)]] for i in ci]
    sel, red = [0], [-math.inf] * 10
    while len(sel) < 4:
        for i in range(10):
            red[i] = max(red[i], O.calculate(COS, cand[i], cand[sel[-1]]))
        rest = [i for i in range(10) if i not in sel]
        sel.append(max(rest, key=lambda i: ((0.5 * cs[i]) - (0.5 * red[i]), -i)))
    expect["mmr"] = (ci[sel], cs[sel])
    # grouped: the ranking walked from the front, a row kept iff its group is new
    seen, keep = set(), []
    for j, i in enumerate(fi.tolist()):
        g = int(gkeys[pos_of[i]])
        if g not in seen:
            seen.add(g)
            keep.append(j)
    keep = keep[:3]
    expect["grouped"] = (fi[keep], fs[keep], [int(gkeys[pos_of[int(i)]]) for i in fi[keep]])
    valid = {"search": dict(k=5), "filtered": dict(k=5), "range": dict(min_score=min_score), "mmr": dict(k=4, fetch_k=10, lam=0.5),
             "grouped": dict(k=3)}

    class W:
        pass
    w = W()
    w.V, w.O, w.ids, w.rows, w.q, w.in_filter, w.gkeys, w.expect, w.valid = V, O, ids, rows, q, in_filter, gkeys, expect, valid
    return w


def make_handle(w, with_nan_row=False, empty=False):
    ids, rows, fids, gids, gk = w.ids, w.rows, w.ids[w.in_filter], w.ids, w.gkeys
    if with_nan_row:  # one more row, in the filter and in a group of its own
        bad = np.full((1, DIM), 0.25)
        bad[0, 3] = np.nan
        ids, rows = np.append(ids, np.uint64(NAN_ID)), np.vstack([rows, bad])
        fids, gids, gk = np.append(fids, np.uint64(NAN_ID)), ids, np.append(gk, np.uint64(5))
    if empty:
        ids, rows = ids[:0], rows[:0]
    return Handle(w.V, ids, rows, fids, gids, gk)


def check_valid(w, h, entry):
    ei, es = w.expect[entry][0], w.expect[entry][1]
    rc, n, total = h.call(entry, w.q, **w.valid[entry])
    assert rc == OK, (entry, rc, h.error())
    assert n == ei.size, (entry, n, ei.size)
    assert h.ids[:n].tolist() == ei.tolist(), entry
    assert bits(h.scores[:n]) == bits(es), entry
    if entry == "range":
        assert total == ei.size
    if entry == "grouped":
        assert h.keys[:n].tolist() == w.expect[entry][2]


def refused(w, h, entry, status, text, **args):
    rc, n, _ = h.call(entry, w.q, **args)
    assert rc == status, (entry, args, rc, h.error())
    assert n == 0, (entry, args, n)
    assert h.error() == text, (entry, args, h.error())
    if status == ERR_DIM_MISMATCH:
        assert h.dim_pair() == (DIM, BAD_LEN), (entry, args)
    check_valid(w, h, entry)  # the handle's next valid call


@pytest.fixture(scope="module")
def handle(world):
    h = make_handle(world)
    for entry in ENTRIES:
        check_valid(world, h, entry)
    return h


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_metric_is_checked_before_the_query_length(world, handle, entry):
    refused(world, handle, entry, ERR_INVALID_ARG, UNKNOWN_METRIC, metric=BAD_METRIC, q_len=BAD_LEN)
    refused(world, handle, entry, ERR_INVALID_ARG, UNKNOWN_METRIC, metric=-1)


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_wrong_query_length_alone(world, handle, entry):
    refused(world, handle, entry, ERR_DIM_MISMATCH, DIM_TEXT, q_len=BAD_LEN)
    if entry != "range":  # the length is checked before k = 0 returns early
        refused(world, handle, entry, ERR_DIM_MISMATCH, DIM_TEXT, q_len=BAD_LEN, k=0, fetch_k=0)


@pytest.mark.parametrize("entry", ENTRIES[1:])
def test_an_unknown_filter_is_reported_before_the_metric(world, handle, entry):
    refused(world, handle, entry, ERR_INVALID_ARG, UNKNOWN_FILTER, token=NO_SUCH, metric=BAD_METRIC)
    refused(world, handle, entry, ERR_INVALID_ARG, UNKNOWN_FILTER, token=NO_SUCH, q_len=BAD_LEN)


def test_range_checks_the_length_before_a_nan_threshold(world, handle):
    refused(world, handle, "range", ERR_DIM_MISMATCH, DIM_TEXT, min_score=math.nan, q_len=BAD_LEN)
    refused(world, handle, "range", ERR_INVALID_ARG, NAN_THRESHOLD, min_score=math.nan)
    refused(world, handle, "range", ERR_INVALID_ARG, UNKNOWN_METRIC, min_score=math.nan, metric=BAD_METRIC)
    refused(world, handle, "range", ERR_INVALID_ARG, UNKNOWN_FILTER, min_score=math.nan, token=NO_SUCH)


def test_grouped_checks_k_then_the_table_then_the_filter_then_the_metric(world, handle):
    refused(world, handle, "grouped", ERR_INVALID_ARG, K_LIMIT, k=1025, groups=NO_SUCH)
    refused(world, handle, "grouped", ERR_INVALID_ARG, UNKNOWN_GROUPS, groups=NO_SUCH, token=NO_SUCH)
    refused(world, handle, "grouped", ERR_INVALID_ARG, UNKNOWN_GROUPS, groups=NO_SUCH, metric=BAD_METRIC)
    refused(world, handle, "grouped", ERR_INVALID_ARG, UNKNOWN_GROUPS, groups=handle.filt.token)  # a filter is no table
    refused(world, handle, "grouped", ERR_INVALID_ARG, UNKNOWN_FILTER, token=handle.table.token)  # ... and the reverse


def test_mmr_checks_its_own_arguments_before_the_filter(world, handle):
    refused(world, handle, "mmr", ERR_INVALID_ARG, "lambda must lie in [0, 1]", lam=1.5, token=NO_SUCH)
    refused(world, handle, "mmr", ERR_INVALID_ARG, "fetch_k must be at least k", k=5, fetch_k=4, token=NO_SUCH)
    refused(world, handle, "mmr", ERR_INVALID_ARG, "fetch_k exceeds VL_MMR_MAX_FETCH (1024)", fetch_k=1025, metric=BAD_METRIC)


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e != "range"])  # (range has no k)
def test_k_zero_is_an_empty_answer(world, handle, entry):
    rc, n, _ = handle.call(entry, world.q, k=0, fetch_k=0)
    assert (rc, n) == (OK, 0), (entry, rc, handle.error())
    check_valid(world, handle, entry)


@pytest.mark.parametrize("entry", ENTRIES)
def test_an_empty_index_accepts_any_query_length(world, entry):
    h = make_handle(world, empty=True)
    rc, n, total = h.call(entry, world.q, q_len=BAD_LEN)
    assert (rc, n) == (OK, 0), (entry, rc, h.error())
    assert total in (None, 0)
    # ... but not any token or metric: those are checked before the index is looked at; the next valid call is an empty answer
    rc, n, _ = h.call(entry, world.q, q_len=BAD_LEN, metric=BAD_METRIC)
    assert (rc, n, h.error()) == (ERR_INVALID_ARG, 0, UNKNOWN_METRIC), entry
    assert h.call(entry, world.q, **world.valid[entry])[:2] == (OK, 0), entry
    if entry != "search":
        rc, n, _ = h.call(entry, world.q, q_len=BAD_LEN, token=NO_SUCH)
        assert (rc, n, h.error()) == (ERR_INVALID_ARG, 0, UNKNOWN_FILTER), entry
        assert h.call(entry, world.q, **world.valid[entry])[:2] == (OK, 0), entry


def test_a_nan_score_on_the_exact_route_and_the_search_after_the_row_is_gone(world):
    h = make_handle(world, with_nan_row=True)  # a NaN row is outside the fast-path domain: every call takes the exact route
    for entry in ENTRIES:
        rc, n, _ = h.call(entry, world.q, **world.valid[entry])
        assert rc == ERR_NAN_SCORE, (entry, rc, h.error())
        assert n == 0 and h.error() == NAN_SCORE, (entry, n, h.error())
    h.idx.delete(NAN_ID)
    for entry in ENTRIES:
        check_valid(world, h, entry)
