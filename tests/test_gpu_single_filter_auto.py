"""The auto single-query filter (vl_index_set_single_filter mode 2, what new handles start in): the bf16 first stage runs on
indexes whose f32 slab is at least 512 MiB and not below, answers exactly what the f32-only mode answers (ids and f64
scores), never costs an MFMA batch straggler a second pass, pauses on a run of uncertifiable queries and comes back."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, EUC, DOT = 0, 1, 3
FLOOR_BYTES = 512 << 20
SCAN16_VARIANT_BASE = 1_000_000


@pytest.fixture(scope="module")
def V():
    import vectorlite_amd as V
    n_dev, _ = V.runtime_info()
    assert n_dev > 0, "GPU tests need a HIP device"
    return V


@pytest.fixture
def no_floor(monkeypatch):
    """Handles created inside the test take the bf16 stage at any size (the floor is read at create)."""
    monkeypatch.setenv("VL_SINGLE_FILTER_MIN_MB", "0")
    monkeypatch.delenv("VL_SINGLE_FILTER", raising=False)


def ldb_of(dim):
    return next(s for s in (128, 256, 384, 512, 768) if dim <= s)


def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def bf16_unit_images(x):
    u = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def planted(rng, n, dim, count=150):
    """n unit rows; `count` of them share ONE bf16 unit image (the base row is +-1/16 per column at dim 256, offsets far
    inside half a bf16 step) while f32 resolves them: the query next to them cannot be certified by a bf16 filter."""
    rows = unit_rows(rng, n, dim)
    b = rng.choice([-1.0, 1.0], size=dim) / np.sqrt(dim)
    q = b + 0.05 * rng.standard_normal(dim) / np.sqrt(dim)
    d = q - (q @ b) * b
    d /= np.abs(d).max()
    eps = 2.0 ** -12 * 0.5 / np.sqrt(dim) / count
    where = np.sort(rng.choice(np.arange(n), size=count, replace=False))
    rows[where] = b[None, :] + (np.arange(1, count + 1) * eps)[:, None] * d[None, :]
    img = bf16_unit_images(rows[where])
    assert (img == img[0]).all(), "construction: the planted rows' bf16 images must be identical"
    return rows, q


def searched(idx, q, k, metric):
    """(ids, scores, scan launches, scan bytes) of one single search."""
    idx.profile_read()
    idx.profile_enable(True)
    i, s = idx.search_arrays(q, k, metric)
    idx.profile_enable(False)
    nl, _, by = idx.profile_read()
    return i.tolist(), s.tolist(), nl, by


def f32_answer(idx, q, k, metric):
    idx.set_single_filter("f32")
    try:
        i, s = idx.search_arrays(q, k, metric)
    finally:
        idx.set_single_filter("auto")
    return i.tolist(), s.tolist()


def device_rows(idx, torch, lo, hi, dim, seed):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    x = torch.randn((hi - lo, dim), dtype=torch.float64, device="cuda:0", generator=g)
    x /= torch.linalg.vector_norm(x, dim=1, keepdim=True)
    idx.add_rows(np.arange(lo, hi, dtype=np.uint64), x, validate=False)
    torch.cuda.synchronize()


def test_auto_engages_above_the_floor_and_not_below(V, monkeypatch):
    """At dim 384 the floor is 349 526 rows (a 512 MiB f32 slab): a scan launch streams n x ld x 4 bytes below it and
    n x ldb x 2 above it; both answers are the f32-only mode's."""
    import torch
    monkeypatch.delenv("VL_SINGLE_FILTER", raising=False)
    monkeypatch.delenv("VL_SINGLE_FILTER_MIN_MB", raising=False)
    dim, ld = 384, 384
    floor_rows = FLOOR_BYTES // (ld * 4)
    idx = V.FlatIndex(dim)
    n = floor_rows - 1
    idx.reserve(floor_rows + 5000)
    device_rows(idx, torch, 0, n, dim, 11)
    Q = unit_rows(np.random.default_rng(3), 6, dim)
    for q in Q[:3]:
        i, s, nl, by = searched(idx, q, 10, COS)
        assert (nl, by) == (1, n * ld * 4), ("below the floor: the f32 scan", nl, by)
        assert idx.last_scan()["variant"] < SCAN16_VARIANT_BASE
        assert (i, s) == f32_answer(idx, q, 10, COS)
    device_rows(idx, torch, n, floor_rows + 4000, dim, 12)  # add: above the floor
    n = floor_rows + 4000
    for q in Q:
        i, s, nl, by = searched(idx, q, 10, COS)
        assert (nl, by) == (1, n * ldb_of(dim) * 2), ("above the floor: the bf16 filter", nl, by)
        ls = idx.last_scan()
        assert ls["variant"] > SCAN16_VARIANT_BASE and ls["query_in_kernarg"] == 1 and ls["grid"] > 0, ls
        assert (i, s) == f32_answer(idx, q, 10, COS)
    for pid in (0, 17, n - 1, 123_456):  # delete: still above, still the same answers
        idx.delete(pid)
    n -= 4
    for q in Q[:3]:
        i, s, nl, by = searched(idx, q, 10, COS)
        assert (nl, by) == (1, n * ldb_of(dim) * 2)
        assert (i, s) == f32_answer(idx, q, 10, COS)
    idx.set_single_filter("f32")  # mode 0 never takes it
    assert searched(idx, Q[0], 10, COS)[3] == n * ld * 4


@pytest.mark.parametrize("dim", [100, 384, 768])
@pytest.mark.parametrize("metric", [COS, DOT, EUC])
def test_auto_answers_equal_the_f32_mode(V, no_floor, dim, metric):
    rng = np.random.default_rng(dim * 10 + metric)
    n = 12000
    rows = unit_rows(rng, n, dim)
    rows[3000:3030] = rows[9] + 1e-4 * rng.standard_normal((30, dim))  # closer than bf16 can resolve
    rows[4000:4010] = rows[21]                                          # exact duplicates: position ties
    ids = np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(1)
    if metric == DOT:
        rows *= rng.uniform(0.5, 2.0, size=(n, 1))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    bf16_only = 0
    for qi in range(8):
        q = rows[9] if qi == 0 else rows[21] if qi == 1 else unit_rows(rng, 1, dim)[0]
        for k in (1, 10, 40):
            i, s, nl, by = searched(idx, q, k, metric)
            assert (i, s) == f32_answer(idx, q, k, metric), (dim, metric, qi, k)
            bf16_only += int(nl == 1 and by == n * ldb_of(dim) * 2)
    assert bf16_only >= 12, bf16_only  # the random queries were answered by the bf16 filter alone


def test_planted_bf16_ties_in_auto_mode(V, no_floor):
    rng = np.random.default_rng(91)
    n, dim = 9000, 256
    rows, q = planted(rng, n, dim)
    idx = V.FlatIndex(dim)
    idx.add_rows(np.arange(n, dtype=np.uint64), rows, validate=False)
    for k in (1, 10, 60):
        i, s, nl, _ = searched(idx, q, k, COS)
        assert nl >= 2, ("the bf16 filter answered the planted query on its own", k, nl)
        assert (i, s) == f32_answer(idx, q, k, COS), k


def test_mfma_stragglers_cost_one_f32_pass(V, no_floor):
    """A query the MFMA batch filter could not certify goes straight to k_scan: the batch costs what it costs with the
    f32-only mode, not one bf16 pass more per straggler."""
    rng = np.random.default_rng(92)
    n, dim = 9000, 256
    rows, q = planted(rng, n, dim)
    idx = V.FlatIndex(dim)
    idx.add_rows(np.arange(n, dtype=np.uint64), rows, validate=False)
    Q = unit_rows(rng, 16, dim)
    Q[5] = q
    out, passes = {}, {}
    for mode in ("f32", "auto", "f32", "auto"):
        idx.set_single_filter(mode)
        idx.profile_read()
        idx.profile_enable(True)
        bi, bs, bn = idx.search_batch(Q, 10, COS)
        idx.profile_enable(False)
        passes.setdefault(mode, []).append(idx.profile_read()[0])
        out.setdefault(mode, []).append((bi.tolist(), bs.tolist(), bn.tolist()))
    assert passes["f32"][0] >= 2, ("construction: the planted query must straggle", passes)
    assert passes["auto"] == passes["f32"], passes
    assert out["auto"][0] == out["f32"][0]
    idx.set_single_filter("auto")
    assert searched(idx, q, 10, COS)[:2] == (out["f32"][0][0][5], out["f32"][0][1][5])


def test_auto_pauses_on_uncertifiable_queries_and_comes_back(V, no_floor):
    rng = np.random.default_rng(93)
    n, dim = 9000, 256
    rows, q = planted(rng, n, dim)
    idx = V.FlatIndex(dim)
    idx.add_rows(np.arange(n, dtype=np.uint64), rows, validate=False)
    ref = f32_answer(idx, q, 10, COS)
    launches = []
    for _ in range(96):
        i, s, nl, _ = searched(idx, q, 10, COS)
        assert (i, s) == ref
        launches.append(nl)
    # on: every planted query pays the bf16 pass and the f32 one; paused after at most 22 of them: one try in 16
    assert all(x == 2 for x in launches[:22]), launches[:22]
    tail = launches[32:]
    assert sum(x - 1 for x in tail) <= len(tail) // 16 + 1, tail
    # certifying queries again: the periodic probes bring it back within 64 probes x 16 searches
    Q = unit_rows(rng, 64, dim)
    for j in range(64 * 16 + 16):
        idx.search_arrays(Q[j % 64], 10, COS)
    for qq in Q[:16]:
        i, s, nl, by = searched(idx, qq, 10, COS)
        assert (nl, by) == (1, n * 256 * 2), "auto did not come back"
        assert (i, s) == f32_answer(idx, qq, 10, COS)


def test_lone_coalesced_caller_and_mutations_between_searches(V, no_floor):
    """search() goes through the coalescer (on by default): a lone caller leads a pass of one, the single-search path.
    Adds and deletes between searches re-convert the bf16 copy's rows on demand; every answer is the f32 mode's."""
    rng = np.random.default_rng(94)
    n, dim = 20000, 384
    rows = unit_rows(rng, n, dim)
    idx = V.FlatIndex(dim)
    idx.add_rows(np.arange(n, dtype=np.uint64), rows, validate=False)
    idx.set_coalescing(16, 0)

    def check(q, ctx):
        i, s = idx.search_arrays(q, 10, COS)
        assert (i.tolist(), s.tolist()) == f32_answer(idx, q, 10, COS), ctx

    Q = unit_rows(rng, 8, dim)
    for j, q in enumerate(Q):
        idx.profile_read()
        idx.profile_enable(True)
        res = idx.search(q, 10)
        idx.profile_enable(False)
        assert idx.profile_read()[2] == n * 384 * 2, "the lone caller took the bf16 filter"
        i, s = f32_answer(idx, q, 10, COS)
        assert [r.id for r in res] == i and [r.score for r in res] == s, j
        check(q, ("lone", j))
    nid = 10 ** 9
    for j in range(3):  # add a row equal to a query, search it; delete a row that was the best answer
        idx.add(V.Vector(nid + j, Q[j] * 1.0))
        i, _ = idx.search_arrays(Q[j], 10, COS)
        assert i[0] == nid + j
        check(Q[j], ("after add", j))
        idx.delete(int(i[1]))
        check(Q[j], ("after delete", j))
        idx.delete(nid + j)
        check(Q[j], ("after deleting the added row", j))
