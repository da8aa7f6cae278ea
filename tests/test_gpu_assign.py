"""Nearest-label assignment (vl_index_assign) against the definition: per stored row,
oracle.FlatOracle(dim, arange(L), labels).search(row, 1, metric).  Labels and score bits are compared; no tolerances."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, EUC, MAN, DOT = 0, 1, 2, 3


@pytest.fixture(scope="module")
def V():
    import vectorlite_amd as V
    n_dev, _ = V.runtime_info()
    assert n_dev > 0, "GPU tests need a HIP device"
    return V


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64).tolist()


@functools.lru_cache(maxsize=4)
def data(dim, n, L, variant=""):
    """Gaussian directions with lengths over 0.25 .. 4, one zero row; labels = noisy copies of random rows with lengths over
    0.5 .. 2, one equal to a stored row, the first one repeated bit for bit as the last (the first and the last chunk).
    Variants: "unit" = unit rows and labels; "tight" = every label a slightly noisy copy of ONE direction, so that no bound
    can tell the labels of a row apart and every pair is a candidate."""
    rng = np.random.default_rng(100000 * dim + 10 * n + L)
    rows = rng.standard_normal((n, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    src = rows[rng.integers(0, n, 1 if variant == "tight" else L)]
    labels = src + (0.02 if variant == "tight" else 0.3) * rng.standard_normal((L, dim)) / np.sqrt(dim)
    labels /= np.linalg.norm(labels, axis=1, keepdims=True)
    if variant != "unit":
        rows *= rng.uniform(0.25, 4.0, (n, 1))
        labels *= rng.uniform(0.5, 2.0, (L, 1))
        rows[n // 2] = 0.0
    if L >= 3:
        labels[L // 2] = rows[5]
    if L >= 2:
        labels[L - 1] = labels[0]
    return np.ascontiguousarray(rows), np.ascontiguousarray(labels)


def oracle_assign(rows, labels, metric):
    from oracle import oracle as O
    ref = O.FlatOracle(labels.shape[1], np.arange(len(labels), dtype=np.uint64), labels)
    got = [ref.search(r, 1, metric) for r in rows]
    return [int(i[0]) for i, _ in got], [float(s[0]) for _, s in got]


@functools.lru_cache(maxsize=4)
def reference(dim, n, L, metric, variant=""):
    return oracle_assign(*data(dim, n, L, variant), metric)


_built = {}


def build(V, dim, n, L, variant=""):
    key = (dim, n, L, variant)
    if key not in _built:
        _built.clear()
        idx = V.FlatIndex(dim)
        idx.add_rows(np.arange(n, dtype=np.uint64) * np.uint64(10) + np.uint64(1), data(*key)[0], validate=False)
        _built[key] = idx
    return _built[key]


def check(V, idx, labels, metric, exp, route="mfma"):
    ids, lab, sc = idx.assign(labels, metric)
    la = idx.last_assign()
    assert la["route"] == route and V.last_path() == (V.PATH_FAST if route == "mfma" else V.PATH_EXACT_SORT), la
    assert ids.tolist() == idx.export()[0].tolist()
    assert lab.tolist() == exp[0], la
    assert bits(sc) == bits(exp[1]), la
    return la


# every stride class, both row counts and 1 / 2 / 3 (and more) label chunks; the chunk is 64 labels, 48 at stride 768
CASES = [(100, 33, 1, COS), (128, 33, 2, EUC), (384, 33, 17, DOT), (768, 33, 97, COS), (100, 4133, 129, EUC), (384, 4133, 128, DOT),
         (384, 4133, 300, COS), (128, 4133, 300, DOT), (768, 4133, 96, EUC), (768, 4133, 200, DOT), (512, 33, 65, EUC), (200, 33, 70, COS)]


@pytest.mark.parametrize("dim,n,L,metric", CASES)
def test_assign_matches_the_oracle_on_the_mfma_route(V, dim, n, L, metric):
    la = check(V, build(V, dim, n, L), data(dim, n, L)[1], metric, reference(dim, n, L, metric))
    assert la["chunks"] == -(-L // (48 if dim > 512 else 64)) and la["split"] == 0 and la["launches"] == 2 * la["ranges"]


def test_the_second_pass_filters(V):
    """Every kept pair lies within 4 E < 0.032 of the row's best cosine (E = IN_EXTRA_MFMA + 2 (n + 4) 2^-24 < 0.008: the
    seed's exact score is within 2 E of the best, a kept pair within 2 E of the seed)."""
    rows, labels = data(384, 4133, 300, "unit")
    la = check(V, build(V, 384, 4133, 300, "unit"), labels, COS, reference(384, 4133, 300, COS, "unit"))
    cos = rows @ labels.T
    assert la["candidates"] <= int((cos >= cos.max(axis=1, keepdims=True) - 0.04).sum()), la


def test_a_small_candidate_buffer_splits_ranges(V, monkeypatch):
    """The tight labels make (nearly) every pair a candidate: 299 per row against a buffer of 32 x 300 pairs (the clamp: one
    block always fits) and first ranges of a quarter of that many rows, so the ranges split down to single blocks."""
    idx = build(V, 384, 4133, 300, "tight")
    monkeypatch.setenv("VL_ASSIGN_CAND_CAP", "1")
    la = check(V, idx, data(384, 4133, 300, "tight")[1], COS, reference(384, 4133, 300, COS, "tight"))
    assert la["split"] > 0 and la["ranges"] > 2 and la["launches"] == 2 * (la["ranges"] + la["split"]), la
    assert la["candidates"] > 100 * 4133, la


def test_exact_route(V):
    rows, labels = data(128, 4133, 129)
    idx = build(V, 128, 4133, 129)
    check(V, idx, labels, MAN, reference(128, 4133, 129, MAN), route="exact")
    fast = idx.assign(labels, EUC)
    assert idx.last_assign()["route"] == "mfma"
    idx.force_path(V.PATH_EXACT_SORT)
    forced = idx.assign(labels, EUC)
    assert idx.last_assign()["route"] == "exact"
    idx.force_path(0)
    idx.set_assign_route("exact")
    asked = idx.assign(labels, EUC)
    assert idx.last_assign()["route"] == "exact"
    idx.set_assign_route("auto")
    for other in (forced, asked):
        assert other[1].tolist() == fast[1].tolist() and bits(other[2]) == bits(fast[2])
    rng = np.random.default_rng(7)
    wide, wl = rng.standard_normal((40, 1000)), rng.standard_normal((5, 1000))
    idx = V.FlatIndex(1000)
    idx.add_rows(np.arange(40, dtype=np.uint64), wide, validate=False)
    check(V, idx, wl, COS, oracle_assign(wide, wl, COS), route="exact")


@pytest.mark.parametrize("route", ["auto", "exact"])
def test_zero_row_under_dot_keeps_the_first_label_and_its_sign(V, route):
    rows = np.vstack([np.zeros((1, 64)), np.ones((1, 64))])
    idx = V.FlatIndex(64)
    idx.add_rows(np.array([3, 4], dtype=np.uint64), rows, validate=False)
    idx.set_assign_route(route)
    ids, lab, sc = idx.assign(np.vstack([-np.ones((1, 64)), np.ones((1, 64))]), DOT)
    assert idx.last_assign()["route"] == ("mfma" if route == "auto" else "exact")
    assert lab.tolist() == [0, 1] and bits(sc) == bits([-0.0, 64.0])


def test_nan_row_then_delete_and_the_answer_follows_the_index(V):
    rows, labels = data(100, 33, 17)
    idx = V.FlatIndex(100)
    idx.add_rows(np.arange(33, dtype=np.uint64), rows, validate=False)
    bad = np.full((1, 100), np.nan)
    idx.add_rows(np.array([99], dtype=np.uint64), bad, validate=False)
    with pytest.raises(V.NaNScore):
        idx.assign(labels, COS)
    idx.delete(99)
    more = data(100, 33, 1)[0][:7]
    idx.add_rows(np.arange(200, 207, dtype=np.uint64), more, validate=False)
    idx.delete_many(np.array([3, 4, 20, 203], dtype=np.uint64))
    ids, vals = idx.export()
    assert len(ids) == 36
    check(V, idx, labels, COS, oracle_assign(vals, labels, COS))


def test_argument_errors_empty_index_and_a_short_output(V):
    rows, labels = data(100, 33, 17)
    idx = V.FlatIndex(100)
    ids, lab, sc = idx.assign(labels[:, :7], COS)  # an empty index accepts any label length
    assert len(ids) == len(lab) == len(sc) == 0 and idx.last_assign()["route"] == 0
    idx.add_rows(np.arange(33, dtype=np.uint64), rows, validate=False)
    exp = reference(100, 33, 17, COS)
    for bad, metric, err in ((np.zeros((0, 7)), 9, V.IndexOpError), (np.zeros((4097, 7)), 9, V.IndexOpError),
                             (labels[:, :7], 9, V.IndexOpError), (labels[:, :7], COS, V.DimensionMismatch)):
        with pytest.raises(err):
            idx.assign(bad, metric)
        check(V, idx, labels, COS, exp)
    out_ids, out_lab, out_sc = (np.full(10, 77, dtype=np.uint64), np.full(10, 77, dtype=np.uint64), np.full(10, 77.0))
    n = C.c_uint64(0)
    rc = idx._L.vl_index_assign(idx._h, labels.ctypes.data, 17, 100, COS, 9, out_ids.ctypes.data, out_lab.ctypes.data,
                                out_sc.ctypes.data, C.byref(n))
    assert rc == 0 and n.value == 9
    assert out_ids.tolist() == list(range(9)) + [77] and out_lab.tolist() == exp[0][:9] + [77]
    assert bits(out_sc) == bits(exp[1][:9] + [77.0])
