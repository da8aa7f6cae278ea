"""The int8 single-query filter (vl_index_set_single_filter mode 3, and the first stage of auto's ladder int8 -> bf16 ->
f32): answers exactly what the f32-only mode answers (ids and f64 scores), streams the int8 rows plus their per-row
scalars in one launch when it certifies, hands uncertifiable queries down the ladder, pauses and comes back, and
certifies the headline distribution at 10 M x 384."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, EUC, DOT = 0, 1, 3
I8_FLOOR_BYTES = 1024 << 20
BF16_FLOOR_BYTES = 512 << 20
SCAN8_VARIANT_BASE = 2_000_000
SCAN16_VARIANT_BASE = 1_000_000


@pytest.fixture(scope="module")
def V():
    import vectorlite_amd as V
    n_dev, _ = V.runtime_info()
    assert n_dev > 0, "GPU tests need a HIP device"
    return V


@pytest.fixture
def no_floors(monkeypatch):
    """Handles created inside the test run the whole ladder at any size (the floors are read at create)."""
    monkeypatch.setenv("VL_SINGLE_FILTER_MIN_MB", "0")
    monkeypatch.setenv("VL_SINGLE_FILTER_I8_MIN_MB", "0")
    monkeypatch.delenv("VL_SINGLE_FILTER", raising=False)


def ldb_of(dim):
    return next(s for s in (128, 256, 384, 512, 768) if dim <= s)


def i8_bytes(n, dim, metric):
    return n * (ldb_of(dim) + 8 + (4 if metric == DOT else 0))


def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def bf16_unit_images(x):
    u = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def near_duplicates(rng, n, dim, count=150):
    """n unit rows; `count` of them share ONE bf16 unit image (offsets far inside half a bf16 step, so far inside the
    int8 rows' residual too) while f32 resolves them: the query next to them can be certified by neither filter."""
    rows = unit_rows(rng, n, dim)
    b = rng.choice([-1.0, 1.0], size=dim) / np.sqrt(dim)
    q = b + 0.05 * rng.standard_normal(dim) / np.sqrt(dim)
    d = q - (q @ b) * b
    d /= np.abs(d).max()
    eps = 2.0 ** -12 * 0.5 / np.sqrt(dim) / count
    where = np.sort(rng.choice(np.arange(n), size=count, replace=False))
    rows[where] = b[None, :] + (np.arange(1, count + 1) * eps)[:, None] * d[None, :]
    img = bf16_unit_images(rows[where])
    assert (img == img[0]).all(), "construction: the near-duplicate rows' bf16 images must be identical"
    return rows, q


def searched(idx, q, k, metric):
    """(ids, scores, scan launches, scan bytes) of one single search."""
    idx.profile_read()
    idx.profile_enable(True)
    i, s = idx.search_arrays(q, k, metric)
    idx.profile_enable(False)
    nl, _, by = idx.profile_read()
    return i.tolist(), s.tolist(), nl, by


def f32_answer(idx, q, k, metric, back="auto"):
    idx.set_single_filter("f32")
    try:
        i, s = idx.search_arrays(q, k, metric)
    finally:
        idx.set_single_filter(back)
    return i.tolist(), s.tolist()


def device_rows(idx, torch, lo, hi, dim, seed):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    x = torch.randn((hi - lo, dim), dtype=torch.float64, device="cuda:0", generator=g)
    x /= torch.linalg.vector_norm(x, dim=1, keepdim=True)
    idx.add_rows(np.arange(lo, hi, dtype=np.uint64), x, validate=False)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dim", [100, 384, 768])
@pytest.mark.parametrize("metric", [COS, DOT])
@pytest.mark.parametrize("mode", ["i8", "auto"])
def test_i8_answers_equal_the_f32_mode(V, no_floors, dim, metric, mode):
    rng = np.random.default_rng(dim * 10 + metric)
    n = 12000
    rows = unit_rows(rng, n, dim)
    rows[3000:3030] = rows[9] + 1e-4 * rng.standard_normal((30, dim))  # closer than int8 can resolve
    rows[4000:4010] = rows[21]                                          # exact duplicates: position ties
    if metric == COS:  # (a 2^38 row would make the dot bound, relative to the largest row norm, useless)
        rows[5000] = 0.0                                                # a zero row
        rows[5001] = 0.0
        rows[5001, 7] = 2.0 ** -39                                       # one-hot rows near the domain's edges
        rows[5002] = 0.0
        rows[5002, 3] = -(2.0 ** 38)
        rows[5003, :] = 2.0 ** 38                                        # large values in every column
    ids = np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(1)
    if metric == DOT:
        rows *= rng.uniform(0.5, 2.0, size=(n, 1))
    idx = V.FlatIndex(dim)
    idx.add_rows(ids, rows, validate=False)
    idx.set_single_filter(mode)
    i8_only = 0
    for qi in range(8):
        q = rows[9] if qi == 0 else rows[21] if qi == 1 else unit_rows(rng, 1, dim)[0]
        for k in (1, 10, 40):
            i, s, nl, by = searched(idx, q, k, metric)
            ls = idx.last_scan()
            assert (i, s) == f32_answer(idx, q, k, metric, mode), (dim, metric, qi, k)
            if nl == 1 and by == i8_bytes(n, dim, metric):
                i8_only += 1
                assert ls["variant"] > SCAN8_VARIANT_BASE and ls["query_in_kernarg"] == 1 and ls["grid"] > 0, ls
    assert i8_only >= 8, i8_only  # the random queries were answered by the int8 filter alone (k = 40 may go on)


def test_euclidean_skips_the_i8_stage(V, no_floors):
    rng = np.random.default_rng(5)
    n, dim = 9000, 384
    rows = unit_rows(rng, n, dim)
    idx = V.FlatIndex(dim)
    idx.add_rows(np.arange(n, dtype=np.uint64), rows, validate=False)
    q = unit_rows(rng, 1, dim)[0]
    i, s, nl, by = searched(idx, q, 10, EUC)
    assert (nl, by) == (1, n * ldb_of(dim) * 2), "auto: Euclidean starts at the bf16 stage"
    assert (i, s) == f32_answer(idx, q, 10, EUC)
    idx.set_single_filter("i8")
    i, s, nl, by = searched(idx, q, 10, EUC)
    assert (nl, by) == (1, n * 384 * 4), "mode i8: Euclidean scans the f32 slab"
    assert (i, s) == f32_answer(idx, q, 10, EUC, "i8")


def test_floors_pick_the_stage(V, monkeypatch):
    """Default floors at dim 384: bf16 between 349 526 and 699 051 rows (a 512 MiB and a 1 GiB f32 slab), int8 above;
    VL_SINGLE_FILTER_MIN_MB does not lower the int8 floor.  One launch each, every answer the f32-only mode's."""
    import torch
    monkeypatch.delenv("VL_SINGLE_FILTER", raising=False)
    monkeypatch.delenv("VL_SINGLE_FILTER_I8_MIN_MB", raising=False)
    monkeypatch.setenv("VL_SINGLE_FILTER_MIN_MB", "0")
    dim = 384
    i8_floor_rows = -(-I8_FLOOR_BYTES // (dim * 4))
    idx = V.FlatIndex(dim)
    n = i8_floor_rows - 1
    idx.reserve(i8_floor_rows + 5000)
    device_rows(idx, torch, 0, n, dim, 21)
    Q = unit_rows(np.random.default_rng(4), 4, dim)
    for q in Q[:2]:
        i, s, nl, by = searched(idx, q, 10, COS)
        assert (nl, by) == (1, n * dim * 2), ("between the floors: the bf16 filter", nl, by)
        assert idx.last_scan()["variant"] < SCAN8_VARIANT_BASE
        assert (i, s) == f32_answer(idx, q, 10, COS)
    device_rows(idx, torch, n, i8_floor_rows + 4000, dim, 22)
    n = i8_floor_rows + 4000
    for q in Q:
        for metric in (COS, DOT):
            i, s, nl, by = searched(idx, q, 10, metric)
            assert (nl, by) == (1, i8_bytes(n, dim, metric)), ("above the int8 floor", metric, nl, by)
            assert idx.last_scan()["variant"] > SCAN8_VARIANT_BASE
            assert (i, s) == f32_answer(idx, q, 10, metric)


def test_floor_knob_at_create(V, monkeypatch):
    monkeypatch.delenv("VL_SINGLE_FILTER", raising=False)
    monkeypatch.setenv("VL_SINGLE_FILTER_MIN_MB", "0")
    monkeypatch.setenv("VL_SINGLE_FILTER_I8_MIN_MB", "20")
    rng = np.random.default_rng(6)
    dim = 256
    rows = unit_rows(rng, 30000, dim)  # 29.3 MiB of f32 slab
    idx = V.FlatIndex(dim)
    idx.add_rows(np.arange(15000, dtype=np.uint64), rows[:15000], validate=False)  # 14.6 MiB: bf16
    q = rows[7] + 0.01 * unit_rows(rng, 1, dim)[0]
    assert searched(idx, q, 10, COS)[2:] == (1, 15000 * 256 * 2)
    idx.add_rows(np.arange(15000, 30000, dtype=np.uint64), rows[15000:], validate=False)
    i, s, nl, by = searched(idx, q, 10, COS)
    assert (nl, by) == (1, i8_bytes(30000, dim, COS))
    assert (i, s) == f32_answer(idx, q, 10, COS)


@pytest.mark.parametrize("mode,launches", [("auto", 3), ("i8", 2)])
def test_near_duplicates_walk_the_ladder(V, no_floors, mode, launches):
    rng = np.random.default_rng(91)
    n, dim = 9000, 256
    rows, q = near_duplicates(rng, n, dim)
    idx = V.FlatIndex(dim)
    idx.add_rows(np.arange(n, dtype=np.uint64), rows, validate=False)
    idx.set_single_filter(mode)
    for k in (1, 10, 60):
        i, s, nl, by = searched(idx, q, k, COS)
        # auto: int8, bf16, f32; mode i8: int8, f32
        assert nl == launches, (mode, k, nl)
        tail = n * 256 * 2 + n * 256 * 4 if mode == "auto" else n * 256 * 4
        assert by == i8_bytes(n, dim, COS) + tail, (mode, k, by)
        assert (i, s) == f32_answer(idx, q, k, COS, mode), k


def test_mfma_stragglers_cost_one_f32_pass(V, no_floors):
    rng = np.random.default_rng(92)
    n, dim = 9000, 256
    rows, q = near_duplicates(rng, n, dim)
    idx = V.FlatIndex(dim)
    idx.add_rows(np.arange(n, dtype=np.uint64), rows, validate=False)
    Q = unit_rows(rng, 16, dim)
    Q[5] = q
    out, passes = {}, {}
    for mode in ("f32", "auto", "i8", "f32", "auto", "i8"):
        idx.set_single_filter(mode)
        idx.profile_read()
        idx.profile_enable(True)
        bi, bs, bn = idx.search_batch(Q, 10, COS)
        idx.profile_enable(False)
        passes.setdefault(mode, []).append(idx.profile_read()[0])
        out.setdefault(mode, []).append((bi.tolist(), bs.tolist(), bn.tolist()))
    assert passes["f32"][0] >= 2, ("construction: the near-duplicate query must straggle", passes)
    assert passes["auto"] == passes["f32"] and passes["i8"] == passes["f32"], passes
    assert out["auto"][0] == out["f32"][0] and out["i8"][0] == out["f32"][0]


def test_window_pauses_and_recovers(V, no_floors):
    rng = np.random.default_rng(93)
    n, dim = 9000, 256
    rows, q = near_duplicates(rng, n, dim)
    idx = V.FlatIndex(dim)
    idx.add_rows(np.arange(n, dtype=np.uint64), rows, validate=False)
    ref = f32_answer(idx, q, 10, COS)
    launches = []
    for _ in range(96):
        i, s, nl, _ = searched(idx, q, 10, COS)
        assert (i, s) == ref
        launches.append(nl)
    # on: each near-duplicate query pays int8 + bf16 + f32; both stages pause after at most 22 failures, then probe
    # one search in 16 each
    assert all(x == 3 for x in launches[:22]), launches[:22]
    tail = launches[32:]
    assert sum(x - 1 for x in tail) <= 2 * (len(tail) // 16 + 1), tail
    Q = unit_rows(rng, 64, dim)
    for j in range(64 * 16 + 16):
        idx.search_arrays(Q[j % 64], 10, COS)
    for qq in Q[:16]:
        i, s, nl, by = searched(idx, qq, 10, COS)
        assert (nl, by) == (1, i8_bytes(n, dim, COS)), "the int8 stage did not come back"
        assert (i, s) == f32_answer(idx, qq, 10, COS)


def test_mode_i8_switches_itself_off(V, no_floors):
    rng = np.random.default_rng(94)
    n, dim = 9000, 256
    rows, q = near_duplicates(rng, n, dim)
    idx = V.FlatIndex(dim)
    idx.add_rows(np.arange(n, dtype=np.uint64), rows, validate=False)
    idx.set_single_filter("i8")
    launches = [searched(idx, q, 10, COS)[2] for _ in range(70)]
    assert launches[:64] == [2] * 64 and launches[64:] == [1] * 6, launches


def test_lone_coalesced_caller_and_mutations_between_searches(V, no_floors):
    """A lone caller of search() (the coalescer, on by default) takes the int8 filter.  Adds, deletes and a capacity
    growth between searches re-convert the int8 copy's rows on demand; every answer is the f32 mode's."""
    rng = np.random.default_rng(95)
    n, dim = 20000, 384
    rows = unit_rows(rng, n, dim)
    idx = V.FlatIndex(dim)
    idx.reserve(n)
    idx.add_rows(np.arange(n, dtype=np.uint64), rows, validate=False)
    idx.set_coalescing(16, 0)

    def check(q, ctx):
        i, s, nl, by = searched(idx, q, 10, COS)
        assert (i, s) == f32_answer(idx, q, 10, COS), ctx
        return nl, by

    Q = unit_rows(rng, 8, dim)
    for j, q in enumerate(Q):
        idx.profile_read()
        idx.profile_enable(True)
        res = idx.search(q, 10)
        idx.profile_enable(False)
        assert idx.profile_read()[2] == i8_bytes(n, dim, COS), "the lone caller took the int8 filter"
        i, s = f32_answer(idx, q, 10, COS)
        assert [r.id for r in res] == i and [r.score for r in res] == s, j
    nid = 10 ** 9
    for j in range(3):  # add a row equal to a query, search it; delete a row that was the best answer
        idx.add(V.Vector(nid + j, Q[j] * 1.0))  # the first add grows the capacity: the copy is freed and rebuilt
        i, _ = idx.search_arrays(Q[j], 10, COS)
        assert i[0] == nid + j
        check(Q[j], ("after add", j))
        idx.delete(int(i[1]))
        check(Q[j], ("after delete", j))
        idx.delete(nid + j)
        assert check(Q[j], ("after deleting the added row", j)) == (1, i8_bytes(idx.len(), dim, COS))


def test_headline_size_fast_equals_exact_and_certifies(V, monkeypatch):
    """10 M x 384 unit rows with default handles (the headline): the int8 stage answers alone, its answers equal the
    exact pipeline's, and it certifies at least 99 % of 1000 headline-distribution queries."""
    import torch
    monkeypatch.delenv("VL_SINGLE_FILTER", raising=False)
    monkeypatch.delenv("VL_SINGLE_FILTER_MIN_MB", raising=False)
    monkeypatch.delenv("VL_SINGLE_FILTER_I8_MIN_MB", raising=False)
    n, dim = 10_000_000, 384
    idx = V.FlatIndex(dim)
    idx.reserve(n)
    for lo in range(0, n, 2_500_000):
        device_rows(idx, torch, lo, lo + 2_500_000, dim, 1000 + lo)
    Q = unit_rows(np.random.default_rng(7), 1000, dim)
    for q in Q[:4]:
        i, s, nl, by = searched(idx, q, 10, COS)
        assert (nl, by) == (1, i8_bytes(n, dim, COS))
        idx.force_path(2)
        try:
            ie, se = idx.search_arrays(q, 10, COS)
        finally:
            idx.force_path(0)
        assert (i, s) == (ie.tolist(), se.tolist())
    certified = 0
    idx.profile_read()
    for q in Q:
        idx.profile_enable(True)
        idx.search_arrays(q, 10, COS)
        idx.profile_enable(False)
        nl, _, by = idx.profile_read()
        certified += int(nl == 1 and by == i8_bytes(n, dim, COS))
    print(f"int8 certification rate at 10 M x 384: {certified}/{len(Q)}")
    assert certified >= 990, certified
