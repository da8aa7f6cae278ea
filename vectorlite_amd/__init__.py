"""vectorlite_amd -- MI355X-native distance-scan engine behind VectorLite's index interface.

Python host-side mirror of the reference's operator interface for the ONE path this repo
implements (reference = mmailhos/vectorlite v0.1.5, paths relative to /root/reference):

    trait VectorIndex            src/lib.rs:224-245     -> FlatIndex.{add, delete, search, len, ...}
    struct Vector / SearchResult src/lib.rs:164-203     -> Vector / SearchResult
    enum SimilarityMetric        src/lib.rs:363-378     -> SimilarityMetric
    VectorLiteError variants     src/errors.rs:18,42    -> DimensionMismatch / MetricMismatch

Every numeric operation happens in libvectorlite_amd.so (HIP kernels, C ABI in
include/vectorlite_amd.h).  This module only marshals buffers and re-attaches text/metadata to
the k winners, which is what a Rust `impl VectorIndex for GpuFlatIndex` would do.
No CPU fallback exists: without the built library, or without a GPU, calls raise.
"""
from __future__ import annotations

import ctypes as C
import enum
import json
import os
import threading
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

__all__ = [
    "SimilarityMetric", "Vector", "SearchResult", "FlatIndex", "MultiFlatIndex", "HNSWIndex", "VectorLiteError", "DimensionMismatch",
    "MetricMismatch", "NaNScore", "DeviceError", "IndexOpError", "IdFilter", "WalkFilter", "GroupTable", "AttrColumn", "hnsw_score", "hnsw_level", "runtime_info",
    "PATH_FAST", "PATH_EXACT_SELECT", "PATH_EXACT_SORT",
]

VL_OK, VL_ERR_DIM_MISMATCH, VL_ERR_DUP_ID, VL_ERR_NOT_FOUND, VL_ERR_METRIC_MISMATCH = 0, 1, 2, 3, 4
VL_ERR_NAN_SCORE, VL_ERR_DEVICE, VL_ERR_OOM, VL_ERR_INVALID_ARG = 5, 6, 7, 8
PATH_NONE, PATH_FAST, PATH_EXACT_SELECT, PATH_EXACT_SORT = 0, 1, 2, 3
VL_MMR_MAX_FETCH = 1024  # most candidates a diversified search ranks (vl_index_search_mmr)
VL_GROUPED_MAX_K = 1024  # most groups a grouped search returns (vl_index_search_grouped)
# set_single_filter: the modes of vl_index_set_single_filter (2 = auto, what new handles start in)
SINGLE_FILTER_MODES = {"f32": 0, "bf16": 1, "auto": 2}
# ... and mode 3, the int8 copy first always (kept out of SINGLE_FILTER_MODES, whose three entries callers enumerate)
SINGLE_FILTER_I8 = 3
# set_masked_batch: the modes of vl_index_set_masked_batch (2 = auto, what new handles start in)
MASKED_BATCH_MODES = {"off": 0, "on": 1, "auto": 2}
WHERE_ROUTES = {"auto": 0, "list": 1, "mask": 2}


class SimilarityMetric(enum.IntEnum):
    """enum SimilarityMetric (src/lib.rs:363-378); Cosine is the default."""
    Cosine = 0
    Euclidean = 1
    Manhattan = 2
    DotProduct = 3

    @classmethod
    def default(cls) -> "SimilarityMetric":
        return cls.Cosine


@dataclass
class Vector:
    """struct Vector (src/lib.rs:164-174)."""
    id: int
    values: Sequence[float]
    text: str = ""
    metadata: Optional[Any] = None


@dataclass
class SearchResult:
    """struct SearchResult (src/lib.rs:194-203)."""
    id: int
    score: float
    text: str = ""
    metadata: Optional[Any] = None


class VectorLiteError(Exception):
    """enum VectorLiteError (src/errors.rs:11-67), the variants a search can return."""


class DimensionMismatch(VectorLiteError):
    def __init__(self, expected: int, actual: int):
        super().__init__(f"Dimension mismatch: expected {expected}, got {actual}")
        self.expected = expected
        self.actual = actual


class MetricMismatch(VectorLiteError):
    def __init__(self, requested, index):
        super().__init__(f"Metric mismatch: requested {requested!r}, index {index!r}")
        self.requested = requested
        self.index = index


class NaNScore(VectorLiteError):
    """Stands in for the reference's panic in `partial_cmp().unwrap()` (src/index/flat.rs:116)."""


class DeviceError(VectorLiteError):
    """HIP runtime failure or no GPU: there is no CPU fallback."""


class IndexOpError(ValueError):
    """add/delete return Err(String) in the reference (src/index/flat.rs:82-96); the message is the
    reference's text ("Vector dimension mismatch", "Vector ID {id} already exists")."""


def _last_error() -> str:
    msg = _lib.load().vl_last_error()
    return msg.decode() if msg else ""


def _raise(rc: int):
    if rc == VL_OK:
        return
    msg = _last_error()
    if rc == VL_ERR_DIM_MISMATCH:
        e, a = C.c_uint64(0), C.c_uint64(0)
        _lib.load().vl_last_dim_mismatch(C.byref(e), C.byref(a))
        raise DimensionMismatch(e.value, a.value)
    if rc == VL_ERR_NAN_SCORE:
        raise NaNScore(msg)
    if rc in (VL_ERR_DEVICE, VL_ERR_OOM):
        raise DeviceError(f"status {rc}: {msg}")
    if rc == VL_ERR_METRIC_MISMATCH:
        raise MetricMismatch(None, None)
    raise VectorLiteError(f"status {rc}: {msg}")


def runtime_info() -> Tuple[int, int]:
    """(number of visible HIP devices, ABI version)."""
    n, v = C.c_int(0), C.c_int(0)
    _lib.load().vl_runtime_info(C.byref(n), C.byref(v))
    return n.value, v.value


def hnsw_score(d_u64: int, metric: int) -> float:
    """convert_distance_to_similarity(d as f64 / 1000.0, metric) (src/index/hnsw.rs:51-75, :478-479)."""
    return _lib.load().vl_hnsw_score(int(d_u64), int(metric))


def hnsw_level(seed: int, node: int, m: int) -> int:
    """The level law (vl_hnsw_level): the top layer, 0 .. 15, of the node at insertion position `node` in an HNSW index
    created with that seed and m.  A builder outside the library lays out its upper lists by it."""
    return int(_lib.load().vl_hnsw_level(int(seed), int(node), int(m)))


def hnsw_levels(seed: int, n: int, m: int) -> np.ndarray:
    """hnsw_level for the nodes 0 .. n - 1 as a uint8 array.  The hash is restated in numpy (exact integer arithmetic);
    a level is taken from numpy's logarithm only where it sits clear of a boundary, otherwise from the library."""
    if n == 0 or m < 2:
        return np.zeros(n, np.uint8)
    with np.errstate(over="ignore"):
        x = np.uint64(seed) * np.uint64(0x100000001B3) + np.arange(n, dtype=np.uint64)
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    u = ((x >> np.uint64(11)).astype(np.float64) + 1.0) * (1.0 / 9007199254740992.0)
    t = -np.log(u) / np.log(float(m))
    lv = np.clip(np.floor(t), 0, 15).astype(np.uint8)
    for i in np.nonzero(np.abs(t - np.rint(t)) < 1e-9)[0]:  # a last-place difference between two logarithms could move these
        lv[i] = hnsw_level(seed, int(i), m)
    return lv


def last_path() -> int:
    return _lib.load().vl_last_path()


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _pf64(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _pu64(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _add_embeddings(L, h, dim: int, ids, embeddings, normalize: bool, validate: bool) -> None:
    """vl_index_add_embeddings_f32: [n, dim] f32 numpy array or torch tensor (a CUDA/HIP tensor on the index's
    device is read in place); widened and L2-normalised on the device as src/embeddings.rs:171-179 does."""
    ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64))
    on_device = False
    try:
        import torch
        is_tensor = isinstance(embeddings, torch.Tensor)
    except Exception:  # pragma: no cover
        is_tensor = False
    if is_tensor and embeddings.is_cuda:
        import torch
        if embeddings.dtype != torch.float32 or not embeddings.is_contiguous():
            raise ValueError("device embeddings must be a contiguous float32 tensor")
        torch.cuda.current_stream(embeddings.device).synchronize()  # producer kernels are done
        ptr, count, on_device = C.c_void_p(embeddings.data_ptr()), embeddings.numel(), True
    else:
        emb = np.ascontiguousarray(np.asarray(embeddings.numpy() if is_tensor else embeddings, dtype=np.float32))
        ptr, count = C.c_void_p(emb.ctypes.data), emb.size
    if count != ids.size * dim:
        raise ValueError("embeddings must be [n, dim]")
    rc = L.vl_index_add_embeddings_f32(h, _pu64(ids), ptr, ids.size, 1 if normalize else 0, 1 if validate else 0,
                                       1 if on_device else 0)
    if rc == VL_ERR_DUP_ID:
        raise IndexOpError(_last_error())
    _raise(rc)


class IdFilter:
    """A set of ids of one FlatIndex (vl_index_filter_create): searches given it rank only the rows whose id is in the set,
    exactly as FlatIndex::search would on an index holding just those rows in their storage order.  It follows the index:
    after add / delete the next use resolves it against the current rows.  `rows()` = rows that qualify now; `close()`
    (or leaving a `with` block) frees it.  An exclusion filter (`make_filter(ids, exclude=True)`,
    vl_index_filter_create_excluding; `exclude` is True) is the opposite set: the rows whose id is NOT in `ids` qualify."""

    def __init__(self, index: "FlatIndex", token: int, exclude: bool = False, columns=None):
        self._index = index
        self._token = token
        self._exclude = bool(exclude)
        self._columns = tuple(columns) if columns is not None else None  # a predicate token keeps its columns referenced

    @property
    def token(self) -> int:
        return self._token

    @property
    def kind(self) -> str:
        """"include", "exclude", or "where" (a predicate token, FlatIndex.make_filter_where)."""
        return "where" if self._columns is not None else "exclude" if self._exclude else "include"

    @property
    def exclude(self) -> bool:
        return self._exclude

    def rows(self) -> int:
        if not self._token:
            raise IndexOpError("filter is closed")
        out = C.c_uint64(0)
        rc = self._index._L.vl_index_filter_rows(self._index._h, self._token, C.byref(out))
        if rc == VL_ERR_INVALID_ARG:
            raise IndexOpError(_last_error())
        _raise(rc)
        return int(out.value)

    def close(self) -> None:
        tok, self._token = self._token, 0
        h = getattr(self._index, "_h", None)
        if tok and h:
            self._index._L.vl_index_filter_destroy(h, tok)

    def __enter__(self) -> "IdFilter":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _make_filter(L, h, owner, ids, exclude: bool = False) -> IdFilter:
    ids = np.ascontiguousarray(np.fromiter((int(i) for i in ids), dtype=np.uint64)
                               if not isinstance(ids, np.ndarray) else ids.astype(np.uint64, copy=False))
    tok, rows = C.c_uint64(0), C.c_uint64(0)
    create = L.vl_index_filter_create_excluding if exclude else L.vl_index_filter_create
    rc = create(h, _pu64(ids), ids.size, C.byref(tok), C.byref(rows))
    if rc == VL_ERR_INVALID_ARG:
        raise IndexOpError(_last_error())
    _raise(rc)
    return IdFilter(owner, int(tok.value), exclude)


class _ExcludeIds:
    """`exclude=` given as an iterable of ids: a one-shot exclusion filter is made of it where the token is needed."""

    def __init__(self, ids):
        self.ids = ids


def _one_filter(filter, exclude):
    """What a search's `filter=` / `exclude=` pair asks for, as the one value _filter_token takes."""
    if exclude is None:
        return filter
    if filter is not None:
        raise ValueError("pass one of filter / exclude")
    if isinstance(exclude, IdFilter):
        if not exclude.exclude:
            raise ValueError("`exclude` takes ids or an exclusion IdFilter (make_filter(ids, exclude=True))")
        return exclude
    return _ExcludeIds(exclude)


class WalkFilter:
    """A set of ids of one HNSWIndex (vl_index_hnsw_filter_create): graph walks given it navigate through every node
    but count only the live nodes whose id is in the set.  It follows the index: after add / delete the next use sees
    the current nodes.  `nodes()` = nodes that pass now; `close()` (or leaving a `with` block) frees it."""

    def __init__(self, index: "HNSWIndex", token: int):
        self._index = index
        self._token = token

    @property
    def token(self) -> int:
        return self._token

    def nodes(self) -> int:
        if not self._token:
            raise IndexOpError("filter is closed")
        out = C.c_uint64(0)
        rc = self._index._L.vl_index_hnsw_filter_nodes(self._index._h, self._token, C.byref(out))
        if rc == VL_ERR_INVALID_ARG:
            raise IndexOpError(_last_error())
        _raise(rc)
        return int(out.value)

    def close(self) -> None:
        tok, self._token = self._token, 0
        h = getattr(self._index, "_h", None)
        if tok and h:
            self._index._L.vl_index_hnsw_filter_destroy(h, tok)

    def __enter__(self) -> "WalkFilter":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GroupTable:
    """A map id -> group key of one FlatIndex (vl_index_groups_create): `search_grouped` returns the best row of each of
    the best k groups; rows whose id the table does not hold take no part.  It follows the index like an IdFilter: after
    add / delete the next use resolves it against the current rows.  `rows()` = rows that have a group now, `distinct()` =
    distinct group keys of the table; `close()` (or leaving a `with` block) frees it."""

    def __init__(self, index: "FlatIndex", token: int):
        self._index = index
        self._token = token

    @property
    def token(self) -> int:
        return self._token

    def _counts(self) -> Tuple[int, int]:
        if not self._token:
            raise IndexOpError("group table is closed")
        rows, distinct = C.c_uint64(0), C.c_uint64(0)
        rc = self._index._L.vl_index_groups_rows(self._index._h, self._token, C.byref(rows), C.byref(distinct))
        if rc == VL_ERR_INVALID_ARG:
            raise IndexOpError(_last_error())
        _raise(rc)
        return int(rows.value), int(distinct.value)

    def rows(self) -> int:
        return self._counts()[0]

    def distinct(self) -> int:
        return self._counts()[1]

    def close(self) -> None:
        tok, self._token = self._token, 0
        h = getattr(self._index, "_h", None)
        if tok and h:
            self._index._L.vl_index_groups_destroy(h, tok)

    def __enter__(self) -> "GroupTable":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _u64_array(values) -> np.ndarray:
    return np.ascontiguousarray(np.fromiter((int(i) for i in values), dtype=np.uint64)
                                if not isinstance(values, np.ndarray) else values.astype(np.uint64, copy=False))


def _i64_array(values) -> np.ndarray:
    return np.ascontiguousarray(np.fromiter((int(i) for i in values), dtype=np.int64)
                                if not isinstance(values, np.ndarray) else values.astype(np.int64, copy=False))


def _pi64(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


class AttrColumn:
    """A map id -> int64 value of one FlatIndex (vl_index_attr_create): `make_filter_where` builds filter tokens from
    range clauses over such columns, resolved on the device.  A row whose id the column does not hold has no value and
    passes no clause; an id the index does not hold waits for a row with that id.  `rows()` = rows that have a value now;
    `set(ids, values)` upserts pairs (tokens made from the column are resolved again on their next use); `close()` (or
    leaving a `with` block) frees the token -- filters made from the column keep working."""

    def __init__(self, index: "FlatIndex", token: int):
        self._index = index
        self._token = token

    @property
    def token(self) -> int:
        return self._token

    def _live(self) -> int:
        if not self._token:
            raise IndexOpError("attribute column is closed")
        return self._token

    def rows(self) -> int:
        out = C.c_uint64(0)
        rc = self._index._L.vl_index_attr_rows(self._index._h, self._live(), C.byref(out))
        if rc == VL_ERR_INVALID_ARG:
            raise IndexOpError(_last_error())
        _raise(rc)
        return int(out.value)

    def set(self, ids, values) -> None:
        ids, values = _u64_array(ids), _i64_array(values)
        if ids.size != values.size:
            raise ValueError("ids and values must have the same length")
        rc = self._index._L.vl_index_attr_set(self._index._h, self._live(), _pu64(ids), _pi64(values), ids.size)
        if rc == VL_ERR_INVALID_ARG:
            raise IndexOpError(_last_error())
        _raise(rc)

    def close(self) -> None:
        tok, self._token = self._token, 0
        h = getattr(self._index, "_h", None)
        if tok and h:
            self._index._L.vl_index_attr_destroy(h, tok)

    def __enter__(self) -> "AttrColumn":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _make_attribute(L, h, owner, ids, values) -> AttrColumn:
    ids, values = _u64_array(ids), _i64_array(values)
    if ids.size != values.size:
        raise ValueError("ids and values must have the same length")
    tok, rows = C.c_uint64(0), C.c_uint64(0)
    rc = L.vl_index_attr_create(h, _pu64(ids), _pi64(values), ids.size, C.byref(tok), C.byref(rows))
    if rc == VL_ERR_INVALID_ARG:
        raise IndexOpError(_last_error())
    _raise(rc)
    return AttrColumn(owner, int(tok.value))


_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1


def _make_filter_where(L, h, owner, clauses, reserved: int = 0) -> IdFilter:
    clauses = list(clauses)
    arr = (_lib.WhereClause * max(len(clauses), 1))()
    columns = []
    for i, cl in enumerate(clauses):
        if len(cl) not in (3, 4):
            raise ValueError("a clause is (column, lo, hi) or (column, lo, hi, negate)")
        col, lo, hi = cl[0], cl[1], cl[2]
        if isinstance(col, AttrColumn):
            if col._index is not owner:
                raise ValueError("the column belongs to another index")
            columns.append(col)
            col = col._live()
        arr[i].attr = int(col)
        arr[i].lo = _I64_MIN if lo is None else int(lo)
        arr[i].hi = _I64_MAX if hi is None else int(hi)
        arr[i].negate = int(cl[3]) if len(cl) == 4 else 0
        arr[i].reserved = reserved
    tok, rows = C.c_uint64(0), C.c_uint64(0)
    rc = L.vl_index_filter_create_where(h, arr, len(clauses), C.byref(tok), C.byref(rows))
    if rc == VL_ERR_INVALID_ARG:
        raise IndexOpError(_last_error())
    _raise(rc)
    return IdFilter(owner, int(tok.value), False, columns)


def _make_groups(L, h, owner, ids, keys) -> GroupTable:
    ids, keys = _u64_array(ids), _u64_array(keys)
    if ids.size != keys.size:
        raise ValueError("ids and keys must have the same length")
    tok, rows = C.c_uint64(0), C.c_uint64(0)
    rc = L.vl_index_groups_create(h, _pu64(ids), _pu64(keys), ids.size, C.byref(tok), C.byref(rows))
    if rc == VL_ERR_INVALID_ARG:
        raise IndexOpError(_last_error())
    _raise(rc)
    return GroupTable(owner, int(tok.value))


def _search_grouped(L, h, query, k: int, metric: int, groups_token: int, filter_token: int):
    """vl_index_search_grouped -> (group_keys, ids, scores), best group first."""
    q = _f64(query).ravel()
    k = min(max(int(k), 0), 1 << 62)
    cap = max(min(k, VL_GROUPED_MAX_K), 1)
    keys = np.empty(cap, dtype=np.uint64)
    ids = np.empty(cap, dtype=np.uint64)
    scores = np.empty(cap, dtype=np.float64)
    n = C.c_uint64(0)
    rc = L.vl_index_search_grouped(h, int(groups_token), int(filter_token), q.ctypes.data, q.size, k, int(metric), cap,
                                   keys.ctypes.data, ids.ctypes.data, scores.ctypes.data, C.byref(n))
    if rc == VL_ERR_INVALID_ARG:
        raise IndexOpError(_last_error())
    _raise(rc)
    m = int(n.value)
    return keys[:m].copy(), ids[:m].copy(), scores[:m].copy()


GROUPED_BATCH_MODES = {"off": 0, "on": 1, "auto": 2}


def _search_grouped_batch(L, h, queries, k: int, metric: int, groups_token: int, filter_token: int):
    """vl_index_search_grouped_batch -> (group_keys [nq, k], ids [nq, k], scores [nq, k], n [nq]); row i holds n[i] entries."""
    Q = np.ascontiguousarray(_f64(queries))
    if Q.ndim != 2:
        raise ValueError("queries must be [nq, dim]")
    nq, q_len = Q.shape
    k = min(max(int(k), 0), 1 << 62)
    stride = min(k, VL_GROUPED_MAX_K)
    keys = np.zeros((nq, stride), dtype=np.uint64)
    ids = np.zeros((nq, stride), dtype=np.uint64)
    scores = np.zeros((nq, stride), dtype=np.float64)
    n = np.zeros(nq, dtype=np.uint64)
    rc = L.vl_index_search_grouped_batch(h, int(groups_token), int(filter_token), Q.ctypes.data, nq, q_len, k, int(metric), stride,
                                         keys.ctypes.data, ids.ctypes.data, scores.ctypes.data, n.ctypes.data)
    if rc == VL_ERR_INVALID_ARG:
        raise IndexOpError(_last_error())
    _raise(rc)
    return keys, ids, scores, n


def _search_range(L, h, query, min_score: float, metric: int, token: int, limit):
    """vl_index_search_range -> (ids, scores, total).  limit=None: everything (the first call's buffers hold 1024 entries;
    a larger total is fetched by a second call sized from the first one's count, repeated if rows arrived in between)."""
    q = _f64(query).ravel()
    cap = 1024 if limit is None else max(int(limit), 0)
    while True:
        ids = np.empty(max(cap, 1), dtype=np.uint64)
        scores = np.empty(max(cap, 1), dtype=np.float64)
        n, total = C.c_uint64(0), C.c_uint64(0)
        rc = L.vl_index_search_range(h, int(token), q.ctypes.data, q.size, float(min_score), int(metric),
                                     ids.ctypes.data if cap else None, scores.ctypes.data if cap else None, cap,
                                     C.byref(n), C.byref(total))
        if rc == VL_ERR_INVALID_ARG:
            raise IndexOpError(_last_error())
        _raise(rc)
        if limit is None and total.value > cap:
            cap = int(total.value)
            continue
        m = int(n.value)
        return ids[:m].copy(), scores[:m].copy(), int(total.value)


def _search_range_batch(L, h, queries, min_score, metric: int, token: int, limit):
    """vl_index_search_range_batch -> (ids_list, scores_list, totals).  limit=None: everything.  The first call's rows hold
    64 entries; the queries whose total is larger -- only those -- are asked again as a second batch with rows sized from
    their largest count (repeated if rows arrived in between).  That second batch's buffers are (overflowing queries) x
    (largest total) x 16 bytes: a caller who expects many low-selectivity queries should pass a `limit`."""
    q = np.ascontiguousarray(_f64(queries))
    if q.ndim != 2:
        raise ValueError("queries must be a 2-d array [nq, dim]")
    nq, dim = q.shape
    ms = np.ascontiguousarray(np.broadcast_to(np.asarray(min_score, dtype=np.float64), (nq,)))

    def call(qs, mss, stride):
        m = qs.shape[0]
        ids = np.empty((m, max(stride, 1)), dtype=np.uint64)
        scores = np.empty((m, max(stride, 1)), dtype=np.float64)
        n = np.zeros(max(m, 1), dtype=np.uint64)
        total = np.zeros(max(m, 1), dtype=np.uint64)
        rc = L.vl_index_search_range_batch(h, int(token), qs.ctypes.data, m, dim, mss.ctypes.data, int(metric), stride,
                                           ids.ctypes.data if stride else None, scores.ctypes.data if stride else None,
                                           n.ctypes.data, total.ctypes.data)
        if rc == VL_ERR_INVALID_ARG:
            raise IndexOpError(_last_error())
        _raise(rc)
        return ([ids[i, :int(n[i])].copy() for i in range(m)], [scores[i, :int(n[i])].copy() for i in range(m)],
                total[:m].astype(np.int64))

    stride = 64 if limit is None else max(int(limit), 0)
    ids_l, scores_l, totals = call(q, ms, stride)
    while limit is None:
        over = np.nonzero(totals > np.array([x.size for x in ids_l], dtype=np.int64))[0]
        if over.size == 0:
            break
        i2, s2, t2 = call(np.ascontiguousarray(q[over]), np.ascontiguousarray(ms[over]), int(totals[over].max()))
        for j, qi in enumerate(over.tolist()):
            ids_l[qi], scores_l[qi], totals[qi] = i2[j], s2[j], t2[j]
    return ids_l, scores_l, totals


def _search_mmr(L, h, query, k: int, fetch_k: int, lambda_mult: float, metric: int, token: int):
    """vl_index_search_mmr -> (ids, scores) in selection order."""
    q = _f64(query).ravel()
    k = min(max(int(k), 0), 1 << 62)
    cap = max(min(k, VL_MMR_MAX_FETCH), 1)
    ids = np.empty(cap, dtype=np.uint64)
    scores = np.empty(cap, dtype=np.float64)
    n = C.c_uint64(0)
    rc = L.vl_index_search_mmr(h, int(token), q.ctypes.data, q.size, k, max(int(fetch_k), 0), float(lambda_mult), int(metric),
                               cap, ids.ctypes.data, scores.ctypes.data, C.byref(n))
    if rc == VL_ERR_INVALID_ARG:
        raise IndexOpError(_last_error())
    _raise(rc)
    m = int(n.value)
    return ids[:m].copy(), scores[:m].copy()


MMR_BATCH_MODES = {"off": 0, "on": 1, "auto": 2}


def _search_mmr_batch(L, h, queries, k: int, fetch_k: int, lambda_mult: float, metric: int, token: int):
    """vl_index_search_mmr_batch -> (ids [nq, stride], scores [nq, stride], n [nq]); row i holds n[i] entries in selection order."""
    Q = np.ascontiguousarray(_f64(queries))
    if Q.ndim != 2:
        raise ValueError("queries must be [nq, dim]")
    nq, q_len = Q.shape
    k = min(max(int(k), 0), 1 << 62)
    stride = min(k, VL_MMR_MAX_FETCH)
    ids = np.zeros((nq, stride), dtype=np.uint64)
    scores = np.zeros((nq, stride), dtype=np.float64)
    n = np.zeros(nq, dtype=np.uint64)
    rc = L.vl_index_search_mmr_batch(h, int(token), Q.ctypes.data, nq, q_len, k, max(int(fetch_k), 0), float(lambda_mult),
                                     int(metric), stride, ids.ctypes.data, scores.ctypes.data, n.ctypes.data)
    if rc == VL_ERR_INVALID_ARG:
        raise IndexOpError(_last_error())
    _raise(rc)
    return ids, scores, n


def _update_rows(L, h, dim: int, ids, values, insert_missing: bool) -> Tuple[int, int]:
    """vl_index_update_bulk -> (rows rewritten, rows appended); the library's refusals as IndexOpError."""
    ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64)).ravel()
    vals = _f64(values)
    if vals.size != ids.size * dim:
        raise ValueError("values must be [n, dim]")
    upd, ins = C.c_uint64(0), C.c_uint64(0)
    rc = L.vl_index_update_bulk(h, _pu64(ids), C.c_void_p(vals.ctypes.data), ids.size, 1 if insert_missing else 0,
                                C.byref(upd), C.byref(ins))
    if rc in (VL_ERR_NOT_FOUND, VL_ERR_INVALID_ARG):
        raise IndexOpError(_last_error())
    _raise(rc)
    return int(upd.value), int(ins.value)


class FlatIndex:
    """GPU-resident counterpart of `FlatIndex` (src/index/flat.rs:60-135).

    `FlatIndex(dim, data)` is `FlatIndex::new(dim, data)`: nothing is validated.
    """

    def __init__(self, dim: int, data: Sequence[Vector] = (), device: int = 0, _handle=None):
        self._L = _lib.load()
        self._meta: Dict[int, Tuple[str, Any]] = {}
        self._h = C.c_void_p()
        self._tls = threading.local()
        self.device = device
        if _handle is not None:
            self._h = _handle
            return
        data = list(data)
        if data:
            ids = np.ascontiguousarray(np.array([v.id for v in data], dtype=np.uint64))
            vals = _f64([list(v.values) for v in data]).reshape(len(data), -1)
            if vals.shape[1] != dim:
                raise ValueError("FlatIndex(dim, data): rows must have `dim` values in this binding")
            _raise(self._L.vl_flat_from_rows(dim, _pu64(ids), _pf64(vals), len(data), device, C.byref(self._h)))
            for v in data:
                self._meta.setdefault(int(v.id), (v.text, v.metadata))
        else:
            _raise(self._L.vl_flat_create(dim, device, C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self._L.vl_index_destroy(h)
            except Exception:
                pass
            self._h = None

    # ---- trait VectorIndex ------------------------------------------------------------------
    def add(self, vector: Vector) -> None:
        vals = _f64(vector.values).ravel()
        rc = self._L.vl_index_add(self._h, int(vector.id), _pf64(vals), vals.size)
        if rc in (VL_ERR_DIM_MISMATCH, VL_ERR_DUP_ID):
            raise IndexOpError(_last_error())
        _raise(rc)
        self._meta[int(vector.id)] = (vector.text, vector.metadata)

    def delete(self, id: int) -> None:
        _raise(self._L.vl_index_delete(self._h, int(id)))
        self._meta.pop(int(id), None)

    def delete_many(self, ids) -> int:
        """`for id in ids: delete(id)` in one call (vl_index_delete_bulk): one walk over the ids and one compaction pass
        over the device arrays, however many ids go.  Absent and repeated ids are ignored.  Returns the rows removed."""
        arr = _u64_array(ids)
        removed = C.c_uint64(0)
        _raise(self._L.vl_index_delete_bulk(self._h, _pu64(arr), arr.size, C.byref(removed)))
        if self._meta:
            for i in arr.tolist():
                self._meta.pop(i, None)
        return int(removed.value)

    def set_delete_bounce(self, nbytes: int) -> None:
        """Bytes of the buffer deletes compact through (0: the default 64 MB); a diagnostic knob (vl_index_set_delete_bounce)."""
        _raise(self._L.vl_index_set_delete_bounce(self._h, int(nbytes)))

    def last_delete(self) -> Dict[str, int]:
        """The last delete_many on this (single-GPU) handle: rows removed and moved, launches that moved a segment in
        place, segments that went through the bounce buffer, bytes written, microseconds on the device."""
        out = (C.c_uint64 * 6)()
        _raise(self._L.vl_index_last_delete(self._h, out))
        return dict(zip(("removed", "moved", "direct_launches", "bounced_segments", "bytes_written", "micros"), (int(v) for v in out)))

    def update(self, vector: Vector) -> None:
        """Replace, in place, the values (and text / metadata) of the first row carrying vector.id (vl_index_update): the row
        keeps its position, every filter / group token its resolved state.  IndexOpError("Vector ID {id} does not exist")
        if no row carries the id; single-GPU flat handles only."""
        vals = _f64(vector.values).ravel()
        rc = self._L.vl_index_update(self._h, int(vector.id), _pf64(vals), vals.size)
        if rc in (VL_ERR_NOT_FOUND, VL_ERR_INVALID_ARG):
            raise IndexOpError(_last_error())
        _raise(rc)
        self._meta[int(vector.id)] = (vector.text, vector.metadata)

    def update_rows(self, ids, values, insert_missing: bool = False) -> Tuple[int, int]:
        """`for id, v in zip(ids, values): update(id, v) if id in index else (add(id, v) if insert_missing else fail)` in
        one call (vl_index_update_bulk), all or nothing: a repeated id keeps its last values, an absent id is appended
        once.  `values`: [n, dim] f64 on the host.  Returns (rows rewritten, rows appended)."""
        return _update_rows(self._L, self._h, self.dimension(), ids, values, insert_missing)

    def upsert_rows(self, ids, values) -> Tuple[int, int]:
        """update_rows(ids, values, insert_missing=True)."""
        return self.update_rows(ids, values, insert_missing=True)

    def last_update(self) -> Dict[str, int]:
        """The last update / update_rows on this (single-GPU) handle: rows rewritten and appended, rows rewritten in the
        row-major bf16, fragment-major bf16 and int8 copies, staging chunks, microseconds on the device."""
        out = (C.c_uint64 * 7)()
        _raise(self._L.vl_index_last_update(self._h, out))
        return dict(zip(("updated", "inserted", "bf16_rows", "bf16_frag_rows", "int8_rows", "chunks", "micros"), (int(v) for v in out)))

    def search(self, query, k: int, similarity_metric: int = SimilarityMetric.Cosine, filter=None,
               exclude=None) -> List[SearchResult]:
        """`filter`: None, an IdFilter of this index, or an iterable of ids (a one-shot filter): the top k among the rows
        whose id is in the set.  `exclude`: an iterable of ids or an exclusion IdFilter: the top k among the rows whose id
        is NOT in the set.  One of the two at most."""
        ids, scores = self.search_arrays(query, k, similarity_metric, filter=filter, exclude=exclude)
        out = []
        for i, s in zip(ids.tolist(), scores.tolist()):
            text, md = self._meta.get(i, ("", None))
            out.append(SearchResult(id=i, score=s, text=text, metadata=md))
        return out

    def len(self) -> int:
        return int(self._L.vl_index_len(self._h))

    __len__ = len

    def is_empty(self) -> bool:
        return bool(self._L.vl_index_is_empty(self._h))

    def dimension(self) -> int:
        return int(self._L.vl_index_dimension(self._h))

    def get_vector(self, id: int) -> Optional[Vector]:
        out = np.empty(max(self.dimension(), 1), dtype=np.float64)
        rc = self._L.vl_index_get_vector(self._h, int(id), _pf64(out))
        if rc == VL_ERR_NOT_FOUND:
            return None
        _raise(rc)
        text, md = self._meta.get(int(id), ("", None))
        return Vector(id=int(id), values=out[: self.dimension()].tolist(), text=text, metadata=md)

    def max_id(self) -> Optional[int]:
        out = C.c_uint64(0)
        rc = self._L.vl_index_max_id(self._h, C.byref(out))
        if rc == VL_ERR_NOT_FOUND:
            return None
        _raise(rc)
        return out.value

    # ---- array-level entry points -----------------------------------------------------------
    def _out_buffers(self, k: int):
        """Per-thread output buffers of the single-query call (ids, scores, count) with their raw addresses:
        made once per thread, regrown only for a larger k.  vl_index_search_cap bounds what the library writes by
        the buffers' own capacity, whatever the index length is by the time the search runs."""
        tl = self._tls
        buf = getattr(tl, "buf", None)
        if buf is None or buf[0] < k:
            cap = max(64, min(int(k), max(self.len(), 1)))
            ids = np.empty(cap, dtype=np.uint64)
            scores = np.empty(cap, dtype=np.float64)
            n = C.c_uint64(0)
            buf = (cap, ids, scores, n, ids.ctypes.data, scores.ctypes.data, C.addressof(n))
            tl.buf = buf
        return buf

    def search_arrays(self, query, k: int, metric: int = 0, filter=None, exclude=None) -> Tuple[np.ndarray, np.ndarray]:
        if exclude is not None:
            filter = _one_filter(filter, exclude)
        q = query
        if not (type(q) is np.ndarray and q.dtype == np.float64 and q.ndim == 1 and q.flags.c_contiguous):
            q = _f64(query).ravel()
        k = min(max(int(k), 0), 1 << 62)
        cap, ids, scores, n, p_ids, p_scores, p_n = self._out_buffers(k)
        if filter is not None:
            return self._search_filtered(q, k, metric, filter, cap, ids, scores, n, p_ids, p_scores, p_n)
        rc = self._L.vl_index_search_cap(self._h, q.ctypes.data, q.size, k, metric, cap, p_ids, p_scores, p_n)
        if rc:
            _raise(rc)
        m = n.value
        return ids[:m].copy(), scores[:m].copy()

    # ---- id filters -------------------------------------------------------------------------
    def make_filter(self, ids, exclude: bool = False) -> IdFilter:
        """An IdFilter over `ids` (any order, repeats allowed; ids the index does not hold are ignored).  exclude=True: the
        rows whose id is NOT in `ids` qualify (an empty `ids` keeps every row; a row added later under one of the ids is
        excluded from then on)."""
        return _make_filter(self._L, self._h, self, ids, exclude)

    # ---- attribute columns and predicate filters -----------------------------------------------
    def make_attribute(self, ids, values) -> AttrColumn:
        """An AttrColumn mapping ids[i] -> values[i] (int64; any order; a pair repeated exactly is fine, an id with two
        different values is an IndexOpError naming the smallest such id)."""
        return _make_attribute(self._L, self._h, self, ids, values)

    def make_filter_where(self, clauses) -> IdFilter:
        """An IdFilter (kind "where") keeping the rows that pass every one of 1 to 4 clauses.  A clause is (column, lo,
        hi) or (column, lo, hi, negate): the row has a value v in the AttrColumn and (lo <= v <= hi) != negate; None as a
        bound is the int64 extreme.  A row without a value passes no clause, negated or not.  The bitmap is computed on the
        device from the columns; the token is passed as `filter=` or inside `filters=[...]` like any other."""
        return _make_filter_where(self._L, self._h, self, clauses)

    def set_where_route(self, mode: str) -> None:
        """How a single search under a predicate token runs: "auto" (new handles: the masked int8 / bf16 / f32 ladder when
        its byte estimate is below the position list's), "list" or "mask".  Answers are identical in every mode."""
        rc = self._L.vl_index_set_where_route(self._h, WHERE_ROUTES[mode])
        if rc == VL_ERR_INVALID_ARG:
            raise IndexOpError("the predicate route is a setting of single-GPU flat indexes")
        _raise(rc)

    def last_where(self) -> Dict[str, int]:
        """The route of the last single predicate-filtered search on this handle (0 list, 1 masked ladder), the rows its
        token kept, and the predicate and column resolutions on this handle so far."""
        v = (C.c_uint64 * 4)()
        _raise(self._L.vl_index_last_where(self._h, v))
        return dict(zip(("route", "m", "resolutions", "column_resolutions"), (int(x) for x in v)))

    def _filter_token(self, filter):
        """(token, one-shot filter to close afterwards or None)"""
        if isinstance(filter, IdFilter):
            if filter._index is not self:
                raise ValueError("the filter belongs to another index")
            return filter.token, None
        f = self.make_filter(filter.ids, exclude=True) if isinstance(filter, _ExcludeIds) else self.make_filter(filter)
        return f.token, f

    def _search_filtered(self, q, k, metric, filter, cap, ids, scores, n, p_ids, p_scores, p_n):
        tok, temp = self._filter_token(filter)
        try:
            rc = self._L.vl_index_search_filtered(self._h, tok, q.ctypes.data, q.size, k, int(metric), cap, p_ids, p_scores, p_n)
        finally:
            if temp is not None:
                temp.close()
        if rc == VL_ERR_INVALID_ARG:
            raise IndexOpError(_last_error())
        _raise(rc)
        m = n.value
        return ids[:m].copy(), scores[:m].copy()

    # ---- range search -----------------------------------------------------------------------
    def search_range_arrays(self, query, min_score: float, metric: int = 0, filter=None, limit=None, exclude=None):
        """(ids, scores, total): every row whose score is >= min_score -- the longest prefix of search(query, len, metric)
        with score >= min_score (among the filter's rows when `filter` is given: an IdFilter or an iterable of ids).
        `total` = rows that qualify; `limit` caps what is returned (0: count only), None returns all of them."""
        filter = _one_filter(filter, exclude)
        if filter is None:
            return _search_range(self._L, self._h, query, min_score, metric, 0, limit)
        tok, temp = self._filter_token(filter)
        try:
            return _search_range(self._L, self._h, query, min_score, metric, tok, limit)
        finally:
            if temp is not None:
                temp.close()

    def search_range(self, query, min_score: float, similarity_metric: int = SimilarityMetric.Cosine, filter=None,
                     limit=None, exclude=None) -> List[SearchResult]:
        ids, scores, _ = self.search_range_arrays(query, min_score, similarity_metric, filter=filter, limit=limit, exclude=exclude)
        out = []
        for i, s in zip(ids.tolist(), scores.tolist()):
            text, md = self._meta.get(i, ("", None))
            out.append(SearchResult(id=i, score=s, text=text, metadata=md))
        return out

    def search_range_batch_arrays(self, queries, min_score, metric: int = 0, filter=None, limit=None, exclude=None):
        """(ids_list, scores_list, totals) for queries [nq, dim]: entry i is search_range_arrays(queries[i], min_score[i], ...)
        on one index state.  `min_score` is a scalar or one value per query; `limit` caps what is returned per query
        (0: count only), None returns every qualifying row.  With limit=None the queries with more than 64 qualifying rows
        are asked a second time: if a writer runs between the two calls they are answered on a later index state than the
        rest of the batch -- pass a `limit` where one state for the whole batch matters."""
        filter = _one_filter(filter, exclude)
        if filter is None:
            return _search_range_batch(self._L, self._h, queries, min_score, metric, 0, limit)
        tok, temp = self._filter_token(filter)
        try:
            return _search_range_batch(self._L, self._h, queries, min_score, metric, tok, limit)
        finally:
            if temp is not None:
                temp.close()

    def search_range_batch(self, queries, min_score, similarity_metric: int = SimilarityMetric.Cosine, filter=None,
                           limit=None, exclude=None) -> List[List[SearchResult]]:
        ids_list, scores_list, _ = self.search_range_batch_arrays(queries, min_score, similarity_metric, filter=filter, limit=limit,
                                                                  exclude=exclude)
        out = []
        for ids, scores in zip(ids_list, scores_list):
            row = []
            for i, s in zip(ids.tolist(), scores.tolist()):
                text, md = self._meta.get(i, ("", None))
                row.append(SearchResult(id=i, score=s, text=text, metadata=md))
            out.append(row)
        return out

    def last_range_batch(self):
        """Routing of the last search_range_batch on this handle: queries answered by the MFMA pass, by the single-query
        fast route, by the exact route, and the largest candidate count the MFMA pass kept for one query."""
        a, b, c, d = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _raise(self._L.vl_index_last_range_batch(self._h, C.byref(a), C.byref(b), C.byref(c)))
        _raise(self._L.vl_index_last_range_batch_candidates(self._h, C.byref(d)))
        return {"mfma_queries": int(a.value), "single_queries": int(b.value), "exact_queries": int(c.value),
                "max_candidates": int(d.value)}

    # ---- grouped search (best row per group) --------------------------------------------------
    def make_groups(self, ids, keys) -> GroupTable:
        """A GroupTable mapping ids[i] -> keys[i] (u64 group keys; any order; an id repeated with the same key is fine, with
        two different keys it is an IndexOpError; ids the index does not hold are ignored)."""
        return _make_groups(self._L, self._h, self, ids, keys)

    def search_grouped_arrays(self, query, k: int, metric: int = 0, groups=None, filter=None, exclude=None):
        """(group_keys, ids, scores): the best row of each of the best k groups of `groups` (a GroupTable of this index), in
        FlatIndex::search's order (among the filter's rows when `filter` is given: an IdFilter or an iterable of ids).
        Rows whose id the table does not hold take no part."""
        filter = _one_filter(filter, exclude)
        if not isinstance(groups, GroupTable):
            raise ValueError("groups must be a GroupTable of this index (make_groups)")
        if groups._index is not self:
            raise ValueError("the group table belongs to another index")
        if filter is None:
            return _search_grouped(self._L, self._h, query, k, metric, groups.token, 0)
        tok, temp = self._filter_token(filter)
        try:
            return _search_grouped(self._L, self._h, query, k, metric, groups.token, tok)
        finally:
            if temp is not None:
                temp.close()

    def search_grouped(self, query, k: int, similarity_metric: int = SimilarityMetric.Cosine, groups=None,
                       filter=None, exclude=None) -> List[Tuple[int, SearchResult]]:
        keys, ids, scores = self.search_grouped_arrays(query, k, similarity_metric, groups=groups, filter=filter, exclude=exclude)
        out = []
        for g, i, s in zip(keys.tolist(), ids.tolist(), scores.tolist()):
            text, md = self._meta.get(i, ("", None))
            out.append((g, SearchResult(id=i, score=s, text=text, metadata=md)))
        return out

    def search_grouped_batch_arrays(self, queries, k: int, metric: int = 0, groups=None, filter=None, exclude=None):
        """(group_keys [nq, k], ids [nq, k], scores [nq, k], n [nq]) for queries [nq, dim]: the first n[i] entries of row i
        are search_grouped_arrays(queries[i], k, ...), all rows on one index state.  Eligible batches share passes of the
        bf16 MFMA batch filter (set_grouped_batch); answers are identical on every route."""
        filter = _one_filter(filter, exclude)
        if not isinstance(groups, GroupTable):
            raise ValueError("groups must be a GroupTable of this index (make_groups)")
        if groups._index is not self:
            raise ValueError("the group table belongs to another index")
        if filter is None:
            return _search_grouped_batch(self._L, self._h, queries, k, metric, groups.token, 0)
        tok, temp = self._filter_token(filter)
        try:
            return _search_grouped_batch(self._L, self._h, queries, k, metric, groups.token, tok)
        finally:
            if temp is not None:
                temp.close()

    def search_grouped_batch(self, queries, k: int, similarity_metric: int = SimilarityMetric.Cosine, groups=None,
                             filter=None, exclude=None) -> List[List[Tuple[int, SearchResult]]]:
        keys, ids, scores, n = self.search_grouped_batch_arrays(queries, k, similarity_metric, groups=groups, filter=filter,
                                                                exclude=exclude)
        out = []
        for r in range(len(n)):
            m = int(n[r])
            row = []
            for g, i, s in zip(keys[r, :m].tolist(), ids[r, :m].tolist(), scores[r, :m].tolist()):
                text, md = self._meta.get(i, ("", None))
                row.append((g, SearchResult(id=i, score=s, text=text, metadata=md)))
            out.append(row)
        return out

    def set_grouped_batch(self, mode: str) -> None:
        """How search_grouped_batch answers an eligible batch: "off" (a loop over the single grouped search under one
        lock), "on" (one bf16 MFMA pass per launch sequence, each query's candidates ranked and collapsed to one row per
        group on the device; what the pass does not settle goes to the single search) or "auto" (new handles: the pass
        when its estimated time is below the loop's).  Answers are identical in every mode."""
        _raise(self._L.vl_index_set_grouped_batch(self._h, GROUPED_BATCH_MODES[mode]))

    def last_grouped_batch(self) -> Dict[str, int]:
        """Of the last search_grouped_batch on this handle: queries sent to the MFMA pass, those it settled, those it handed
        back to the single search, and its launch sequences; all zero when the call looped."""
        v = [C.c_uint64(0) for _ in range(4)]
        _raise(self._L.vl_index_last_grouped_batch(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("routed", "settled", "handed_back", "sequences"), (int(x.value) for x in v)))

    # ---- diversified (MMR) search ------------------------------------------------------------
    def search_mmr_arrays(self, query, k: int, fetch_k: int = 20, lambda_mult: float = 0.5, metric: int = 0, filter=None, exclude=None):
        """(ids, scores): maximal marginal relevance over the exact candidates search(query, fetch_k, metric) (among the
        filter's rows when `filter` is given: an IdFilter or an iterable of ids).  The best candidate first, then k - 1
        times the one maximising lambda_mult * score - (1 - lambda_mult) * (largest similarity to anything chosen);
        entries come in selection order, scores are the candidates' search scores.  lambda_mult = 1 is the plain top k."""
        filter = _one_filter(filter, exclude)
        if filter is None:
            return _search_mmr(self._L, self._h, query, k, fetch_k, lambda_mult, metric, 0)
        tok, temp = self._filter_token(filter)
        try:
            return _search_mmr(self._L, self._h, query, k, fetch_k, lambda_mult, metric, tok)
        finally:
            if temp is not None:
                temp.close()

    def search_mmr(self, query, k: int, fetch_k: int = 20, lambda_mult: float = 0.5,
                   similarity_metric: int = SimilarityMetric.Cosine, filter=None, exclude=None) -> List[SearchResult]:
        ids, scores = self.search_mmr_arrays(query, k, fetch_k, lambda_mult, similarity_metric, filter=filter, exclude=exclude)
        out = []
        for i, s in zip(ids.tolist(), scores.tolist()):
            text, md = self._meta.get(i, ("", None))
            out.append(SearchResult(id=i, score=s, text=text, metadata=md))
        return out

    def search_mmr_batch_arrays(self, queries, k: int, fetch_k: int = 20, lambda_mult: float = 0.5, metric: int = 0, filter=None,
                                exclude=None):
        """(ids [nq, k], scores [nq, k], n [nq]) for queries [nq, dim]: the first n[i] entries of row i are
        search_mmr_arrays(queries[i], k, fetch_k, lambda_mult, ...), all rows on one index state.  Eligible batches share
        passes of the bf16 MFMA batch filter (set_mmr_batch); answers are identical on every route."""
        filter = _one_filter(filter, exclude)
        if filter is None:
            return _search_mmr_batch(self._L, self._h, queries, k, fetch_k, lambda_mult, metric, 0)
        tok, temp = self._filter_token(filter)
        try:
            return _search_mmr_batch(self._L, self._h, queries, k, fetch_k, lambda_mult, metric, tok)
        finally:
            if temp is not None:
                temp.close()

    def search_mmr_batch(self, queries, k: int, fetch_k: int = 20, lambda_mult: float = 0.5,
                         similarity_metric: int = SimilarityMetric.Cosine, filter=None, exclude=None) -> List[List[SearchResult]]:
        ids, scores, n = self.search_mmr_batch_arrays(queries, k, fetch_k, lambda_mult, similarity_metric, filter=filter,
                                                      exclude=exclude)
        out = []
        for r in range(len(n)):
            m = int(n[r])
            row = []
            for i, s in zip(ids[r, :m].tolist(), scores[r, :m].tolist()):
                text, md = self._meta.get(i, ("", None))
                row.append(SearchResult(id=i, score=s, text=text, metadata=md))
            out.append(row)
        return out

    def set_mmr_batch(self, mode: str) -> None:
        """How search_mmr_batch answers an eligible batch: "off" (a loop over the single diversified search under one
        lock), "on" (one bf16 MFMA pass per launch sequence, each query's certified candidates compared and selected on the
        device; what the pass does not settle goes to the single search) or "auto" (new handles: the pass when its
        estimated time is below the loop's).  Answers are identical in every mode."""
        _raise(self._L.vl_index_set_mmr_batch(self._h, MMR_BATCH_MODES[mode]))

    def last_mmr_batch(self) -> Dict[str, int]:
        """Of the last search_mmr_batch on this handle: queries sent to the MFMA pass, those it settled, those it handed
        back to the single search, and its launch sequences; all zero when the call looped."""
        v = [C.c_uint64(0) for _ in range(4)]
        _raise(self._L.vl_index_last_mmr_batch(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("routed", "settled", "handed_back", "sequences"), (int(x.value) for x in v)))

    def search_positions(self, query, k: int, metric: int = 0):
        """(positions, ids, scores): positions are storage positions, for row-shard merging."""
        q = _f64(query).ravel()
        m = max(min(int(k), self.len()), 1)
        pos = np.empty(m, dtype=np.uint64)
        ids = np.empty(m, dtype=np.uint64)
        scores = np.empty(m, dtype=np.float64)
        n = C.c_uint64(0)
        _raise(self._L.vl_index_search_positions(self._h, _pf64(q), q.size, min(int(k), m), int(metric), _pu64(pos),
                                                 _pu64(ids), _pf64(scores), C.byref(n)))
        return pos[: n.value].copy(), ids[: n.value].copy(), scores[: n.value].copy()

    def search_batch(self, queries, k: int, metric: int = 0, filter=None, filters=None, exclude=None):
        """New capability (no reference counterpart): nq independent searches.  `exclude` (ids or an exclusion IdFilter)
        stands where `filter` does; the items of `filters` may be IdFilters of either kind.
        Returns (ids [nq, k], scores [nq, k], n [nq]); row i is exactly search(queries[i]) (with `filter`: exactly
        search(queries[i], filter=filter); with `filters`, a sequence of nq items each an IdFilter of this index or an
        iterable of ids: exactly search(queries[i], filter=filters[i])).  The filtered forms share scan launches
        (last_filtered_batch() tells how the jobs were routed)."""
        filter = _one_filter(filter, exclude)
        if filter is not None and filters is not None:
            raise ValueError("give `filter` (one for the batch) or `filters` (one per query), not both")
        Q = _f64(queries)
        if Q.ndim != 2:
            raise ValueError("queries must be [nq, dim]")
        nq, qlen = Q.shape
        if filters is not None:
            filters = list(filters)
            if len(filters) != nq:
                raise ValueError("`filters` must hold one filter per query (%d queries, %d filters)" % (nq, len(filters)))
        kk = max(min(int(k), self.len()), 1)   # min(k, len) results at most; k is clamped to the buffers
        kc = min(int(k), kk)
        ids = np.zeros((nq, kk), dtype=np.uint64)
        scores = np.zeros((nq, kk), dtype=np.float64)
        n = np.zeros(max(nq, 1), dtype=np.uint64)
        if filters is not None:
            temps = []
            try:
                toks = np.zeros(max(nq, 1), dtype=np.uint64)
                for i, f in enumerate(filters):
                    tok, temp = self._filter_token(f)
                    if temp is not None:
                        temps.append(temp)
                    toks[i] = tok
                rc = self._L.vl_index_search_batch_filters(self._h, _pu64(toks), nq, _pf64(Q), nq, qlen, kc, int(metric), kk,
                                                           _pu64(ids), _pf64(scores), _pu64(n))
            finally:
                for temp in temps:
                    temp.close()
            if rc == VL_ERR_INVALID_ARG:
                raise IndexOpError(_last_error())
            _raise(rc)
            return ids[:, :kc], scores[:, :kc], n[:nq]
        if filter is not None:
            tok, temp = self._filter_token(filter)
            try:
                rc = self._L.vl_index_search_batch_filtered(self._h, tok, _pf64(Q), nq, qlen, kc, int(metric), kk, _pu64(ids),
                                                            _pf64(scores), _pu64(n))
            finally:
                if temp is not None:
                    temp.close()
            if rc == VL_ERR_INVALID_ARG:
                raise IndexOpError(_last_error())
            _raise(rc)
            return ids[:, :kc], scores[:, :kc], n[:nq]
        _raise(self._L.vl_index_search_batch(self._h, _pf64(Q), nq, qlen, kc, int(metric), _pu64(ids),
                                             _pf64(scores), _pu64(n)))
        return ids[:, :kc], scores[:, :kc], n[:nq]

    def last_filtered_batch(self) -> Dict[str, int]:
        """Routing of the last filtered search_batch on this handle: jobs (query, filter pairs) answered by a batched
        launch, jobs handed to the single filtered search before any launch, jobs a batched launch could not certify
        (redone on the exact kernels), and the batched scan launches.  Jobs with an empty subset count nowhere."""
        a, b, c, d = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _raise(self._L.vl_index_last_filtered_batch(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"batched": int(a.value), "single": int(b.value), "exact": int(c.value), "launches": int(d.value)}

    def set_masked_batch(self, mode: str) -> None:
        """How a filtered search_batch answers queries under exclusion tokens: "off" (with the jobs launches, like
        include tokens), "on" (every eligible query with the mask-aware MFMA batch pass: one pass over the bf16 rows per
        launch sequence, each query under its own token's keep bitmap, no position list) or "auto" (new handles: the
        pass when its estimated time is below the jobs launches').  Answers are identical in every mode."""
        _raise(self._L.vl_index_set_masked_batch(self._h, MASKED_BATCH_MODES[mode]))

    def last_masked_batch(self) -> Dict[str, int]:
        """Of the last filtered search_batch on this handle: queries sent to the mask-aware MFMA pass, those it answered,
        those it handed back to the jobs (last_filtered_batch() counts them; it counts none of the answered ones), the
        pass's launch sequences, and the position lists of exclusion tokens the call had to build."""
        v = [C.c_uint64(0) for _ in range(5)]
        _raise(self._L.vl_index_last_masked_batch(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("routed", "certified", "redone", "sequences", "lists_built"), (int(x.value) for x in v)))

    def search_batch_device(self, queries, k: int, metric: int = 0, with_positions: bool = False):
        """search_batch for queries that are already on this index's GPU: `queries` is a contiguous float64 torch tensor
        [nq, dim] on that device (vl_index_search_batch_dev: no host staging, no PCIe copy of the queries on the MFMA
        batch path).  Returns (ids, scores, n), or (positions, ids, scores, n) with `with_positions`."""
        import torch
        if not isinstance(queries, torch.Tensor) or queries.dtype != torch.float64 or not queries.is_contiguous() \
                or queries.dim() != 2 or not queries.is_cuda:
            raise ValueError("queries must be a contiguous float64 [nq, dim] tensor on the index's GPU")
        nq, qlen = queries.shape
        kk = max(min(int(k), self.len()), 1)
        kc = min(int(k), kk)
        pos = np.zeros((nq, kk), dtype=np.uint64) if with_positions else None
        ids = np.zeros((nq, kk), dtype=np.uint64)
        scores = np.zeros((nq, kk), dtype=np.float64)
        n = np.zeros(max(nq, 1), dtype=np.uint64)
        torch.cuda.current_stream(queries.device).synchronize()  # whatever produced the queries has finished
        _raise(self._L.vl_index_search_batch_dev(self._h, C.c_void_p(queries.data_ptr()), nq, qlen, kc, int(metric),
                                                 _pu64(pos) if with_positions else None, _pu64(ids), _pf64(scores), _pu64(n)))
        if with_positions:
            return pos[:, :kc], ids[:, :kc], scores[:, :kc], n[:nq]
        return ids[:, :kc], scores[:, :kc], n[:nq]

    def search_batch_embeddings(self, embeddings, k: int, metric: int = 0, normalize: bool = True):
        """The caller's embed -> search step for a batch (src/client.rs:393-401): `embeddings` is [nq, dim] float32 as the
        model emits it -- a numpy array, or a contiguous torch tensor on this index's GPU.  Widening to f64 and the L2
        normalisation of src/embeddings.rs:169-181 run on the device, bit for bit, then vl_index_search_batch_dev.
        Returns (ids, scores, n) like search_batch."""
        on_device = False
        try:
            import torch
            is_tensor = isinstance(embeddings, torch.Tensor)
        except Exception:  # pragma: no cover
            is_tensor = False
        if is_tensor:
            import torch
            if embeddings.dtype != torch.float32 or not embeddings.is_contiguous() or embeddings.dim() != 2:
                raise ValueError("embeddings must be a contiguous float32 [nq, dim] tensor")
            if embeddings.is_cuda:
                on_device = True
                torch.cuda.current_stream(embeddings.device).synchronize()
                ptr = C.c_void_p(embeddings.data_ptr())
                nq, dim = embeddings.shape
            else:
                embeddings = embeddings.numpy()
        if not on_device:
            E = np.ascontiguousarray(np.asarray(embeddings, dtype=np.float32))
            if E.ndim != 2:
                raise ValueError("embeddings must be [nq, dim]")
            nq, dim = E.shape
            ptr = C.c_void_p(E.ctypes.data)
        kk = max(min(int(k), self.len()), 1)
        kc = min(int(k), kk)
        ids = np.zeros((nq, kk), dtype=np.uint64)
        scores = np.zeros((nq, kk), dtype=np.float64)
        n = np.zeros(max(nq, 1), dtype=np.uint64)
        _raise(self._L.vl_index_search_batch_embeddings_f32(self._h, ptr, nq, dim, 1 if normalize else 0, 1 if on_device else 0,
                                                            kc, int(metric), _pu64(ids), _pf64(scores), _pu64(n)))
        return ids[:, :kc], scores[:, :kc], n[:nq]

    def search_batch_positions(self, queries, k: int, metric: int = 0):
        """(positions, ids, scores, n), each [nq, k] ([nq] for n): the batched search_positions."""
        Q = _f64(queries)
        if Q.ndim != 2:
            raise ValueError("queries must be [nq, dim]")
        nq, qlen = Q.shape
        kk = max(min(int(k), self.len()), 1)
        kc = min(int(k), kk)
        pos = np.zeros((nq, kk), dtype=np.uint64)
        ids = np.zeros((nq, kk), dtype=np.uint64)
        scores = np.zeros((nq, kk), dtype=np.float64)
        n = np.zeros(max(nq, 1), dtype=np.uint64)
        _raise(self._L.vl_index_search_batch_positions(self._h, _pf64(Q), nq, qlen, kc, int(metric), _pu64(pos),
                                                       _pu64(ids), _pf64(scores), _pu64(n)))
        return pos[:, :kc], ids[:, :kc], scores[:, :kc], n[:nq]

    def add_rows(self, ids, values, validate: bool = True) -> None:
        """n x add() in one device pass.  `values`: [n, dim] f64 numpy array, or a torch CUDA/HIP
        tensor (f64, contiguous, on this index's device) which is ingested device-to-device."""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64))
        n = ids.size
        on_device = False
        try:
            import torch
            is_tensor = isinstance(values, torch.Tensor)
        except Exception:  # pragma: no cover
            is_tensor = False
        if is_tensor:
            import torch
            if values.dtype != torch.float64 or not values.is_contiguous():
                raise ValueError("device rows must be a contiguous float64 tensor")
            if values.numel() != n * self.dimension():
                raise ValueError("values must be [n, dim]")
            if values.is_cuda:
                torch.cuda.current_stream(values.device).synchronize()  # producer kernels are done
                on_device = True
                ptr = C.c_void_p(values.data_ptr())
            else:
                values = values.numpy()
        if not on_device:
            vals = _f64(values)
            if vals.size != n * self.dimension():
                raise ValueError("values must be [n, dim]")
            ptr = C.c_void_p(vals.ctypes.data)
        rc = self._L.vl_index_add_bulk(self._h, _pu64(ids), ptr, n, 1 if validate else 0, 1 if on_device else 0)
        if rc == VL_ERR_DUP_ID:
            raise IndexOpError(_last_error())
        _raise(rc)

    def add_embeddings(self, ids, embeddings, normalize: bool = True, validate: bool = True) -> None:
        """The ingest step in front of add (src/embeddings.rs:169-181 then src/index/flat.rs:82-91 per row): f32
        model output -> normalised f64 rows on the device -> n x add()."""
        _add_embeddings(self._L, self._h, self.dimension(), ids, embeddings, normalize, validate)

    def reserve(self, n_rows: int) -> None:
        _raise(self._L.vl_index_reserve(self._h, int(n_rows)))

    def clone(self) -> "FlatIndex":
        h = C.c_void_p()
        _raise(self._L.vl_index_clone(self._h, C.byref(h)))
        c = FlatIndex(self.dimension(), device=self.device, _handle=h)
        c._meta = dict(self._meta)
        return c

    def export(self) -> Tuple[np.ndarray, np.ndarray]:
        n, d = self.len(), self.dimension()
        ids = np.empty(max(n, 1), dtype=np.uint64)
        vals = np.empty((max(n, 1), max(d, 1)), dtype=np.float64)
        _raise(self._L.vl_index_export(self._h, _pu64(ids), _pf64(vals)))
        return ids[:n].copy(), vals[:n, :d].copy()

    def hnsw_distances(self, query, positions, metric: int) -> np.ndarray:
        """Metric::distance(query, row) -> u64 for the rows at `positions` (src/index/hnsw.rs:113-174)."""
        q = _f64(query).ravel()
        pos = np.ascontiguousarray(np.asarray(positions, dtype=np.uint64))
        out = np.empty(max(pos.size, 1), dtype=np.uint64)
        _raise(self._L.vl_index_hnsw_distances(self._h, _pf64(q), q.size, int(metric), _pu64(pos), pos.size,
                                               _pu64(out)))
        return out[: pos.size].copy()

    # ---- diagnostics ------------------------------------------------------------------------
    def force_path(self, path: int) -> None:
        _raise(self._L.vl_index_force_path(self._h, int(path)))

    def set_single_filter(self, mode: str) -> None:
        """Which copy of the slab single queries scan first: "f32" (the f32 slab only), "bf16" (the bf16 copy first,
        always), "i8" (the int8 copy first, always; cosine and dot) or "auto" (new handles: the int8 copy first on
        indexes whose f32 slab is at least 1 GiB, then the bf16 copy on those of at least 512 MiB, each paused while it
        fails to certify).  Answers are identical in every mode."""
        _raise(self._L.vl_index_set_single_filter(self._h, SINGLE_FILTER_I8 if mode == "i8" else SINGLE_FILTER_MODES[mode]))

    def set_coalescing(self, max_batch: int, window_us: int = 0) -> None:
        """Answer concurrent search() calls (other threads) with shared slab passes; 0 turns it off."""
        _raise(self._L.vl_index_set_coalescing(self._h, int(max_batch), int(window_us)))

    def coalesce_stats(self) -> Tuple[int, int]:
        b, q = C.c_uint64(0), C.c_uint64(0)
        _raise(self._L.vl_index_coalesce_stats(self._h, C.byref(b), C.byref(q)))
        return int(b.value), int(q.value)

    def coalesce_gather(self, adaptive: Optional[bool] = None) -> Tuple[int, int]:
        """Switch the coalescer's adaptive gather (None leaves it) and read (passes whose leader waited, microseconds waited)."""
        w, us = C.c_uint64(0), C.c_uint64(0)
        _raise(self._L.vl_index_coalesce_gather(self._h, -1 if adaptive is None else int(bool(adaptive)), C.byref(w), C.byref(us)))
        return int(w.value), int(us.value)

    def last_scan(self) -> Dict[str, int]:
        """Which k_scan instantiation / grid answered the last single search (vl_index_last_scan)."""
        v, g, q = C.c_int(0), C.c_int(0), C.c_int(0)
        _raise(self._L.vl_index_last_scan(self._h, C.byref(v), C.byref(g), C.byref(q)))
        return {"variant": int(v.value), "grid": int(g.value), "query_in_kernarg": int(q.value)}

    def last_filter(self) -> Dict[str, int]:
        """The batch filter's last launch sequence on this handle (vl_index_last_filter)."""
        v = (C.c_int * 6)()
        _raise(self._L.vl_index_last_filter(self._h, v))
        return {"ksteps": v[0], "metric": v[1], "chunks": v[2], "grid_x": v[3], "stages": v[4], "sample_blocks": v[5]}

    def profile_enable(self, on: bool) -> None:
        _raise(self._L.vl_index_profile_enable(self._h, 1 if on else 0))

    def profile_read(self) -> Tuple[int, float, int]:
        n, ms, b = C.c_uint64(0), C.c_double(0.0), C.c_uint64(0)
        _raise(self._L.vl_index_profile_read(self._h, C.byref(n), C.byref(ms), C.byref(b)))
        return n.value, ms.value, b.value


class MultiFlatIndex(FlatIndex):
    """ONE flat index over several GPUs in one process (vl_flat_create_multi): the same `VectorIndex` surface as
    `FlatIndex`, every method inherited -- only the handle differs.  mode "replicas": every GPU holds every row,
    concurrent searches are dealt to the least busy replica, batches are cut across them.  mode "row_shards": every
    GPU holds part of the rows, every search runs on all of them and the exact per-shard top-k are merged on the
    device, bit-identical to one index holding every row.  A device listed twice = two parts on that card."""

    REPLICAS, ROW_SHARDS = 0, 1

    def __init__(self, dim: int, devices: Sequence[int], mode="replicas"):
        m = {"replicas": 0, "row_shards": 1}.get(mode, mode)
        if m not in (0, 1):
            raise ValueError("mode must be 'replicas' or 'row_shards'")
        L = _lib.load()
        devs = [int(d) for d in devices]
        arr = (C.c_int * max(len(devs), 1))(*devs)
        h = C.c_void_p()
        _raise(L.vl_flat_create_multi(int(dim), arr, len(devs), int(m), C.byref(h)))
        super().__init__(dim, device=devs[0] if devs else 0, _handle=h)
        self.devices = devs
        self.mode = int(m)

    def parts(self) -> Dict[str, Any]:
        """Rows held and searches answered by each part (vl_index_parts)."""
        n, mode = C.c_int(0), C.c_int(0)
        _raise(self._L.vl_index_parts(self._h, C.byref(n), C.byref(mode), None, None, 0))
        rows = np.zeros(max(n.value, 1), dtype=np.uint64)
        srch = np.zeros(max(n.value, 1), dtype=np.uint64)
        _raise(self._L.vl_index_parts(self._h, C.byref(n), C.byref(mode), _pu64(rows), _pu64(srch), int(n.value)))
        return {"n_parts": int(n.value), "mode": int(mode.value), "rows": rows[: n.value].tolist(), "searches": srch[: n.value].tolist()}

    def clone(self) -> "MultiFlatIndex":
        h = C.c_void_p()
        _raise(self._L.vl_index_clone(self._h, C.byref(h)))
        c = MultiFlatIndex.__new__(MultiFlatIndex)
        FlatIndex.__init__(c, self.dimension(), device=self.device, _handle=h)
        c.devices, c.mode = list(self.devices), self.mode
        c._meta = dict(self._meta)
        return c


class HNSWIndex:
    """GPU counterpart of `HNSWIndex` (src/index/hnsw.rs:197-496), default profile M = 16, M0 = 32.

    The distance callbacks (u64 = trunc(dist * 1000)), the score conversion, ef = min(k, len), the
    tombstone deletes and every error are the reference's; the graph walk is this library's own
    (crate hnsw 0.11.0 is not in the reference tree), so results are approximate: judged by recall."""

    def __init__(self, dim: int, metric: int = SimilarityMetric.Cosine, device: int = 0, m: int = 16, m0: int = 32,
                 ef_construction: int = 400, seed: int = 0, _handle=None):
        self._L = _lib.load()
        self._meta: Dict[int, Tuple[str, Any]] = {}
        self._h = C.c_void_p()
        self.device = device
        if _handle is not None:  # adopt a handle made by the library (vl_vlc_build_index)
            self._h = _handle
            return
        if dim == 0:
            raise ValueError("HNSW index dimension cannot be 0")  # panics in the reference (:217-219)
        _raise(self._L.vl_hnsw_create_ex(dim, int(metric), m, m0, ef_construction, seed, device, C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self._L.vl_index_destroy(h)
            except Exception:
                pass
            self._h = None

    def set_coalescing(self, max_batch: int, window_us: int = 0) -> None:
        """Concurrent search() calls (other threads) share graph-walk launches; 0 turns it off."""
        _raise(self._L.vl_index_set_coalescing(self._h, int(max_batch), int(window_us)))

    def coalesce_stats(self) -> Tuple[int, int]:
        b, q = C.c_uint64(0), C.c_uint64(0)
        _raise(self._L.vl_index_coalesce_stats(self._h, C.byref(b), C.byref(q)))
        return int(b.value), int(q.value)

    def coalesce_gather(self, adaptive: Optional[bool] = None) -> Tuple[int, int]:
        """Switch the coalescer's adaptive gather (None leaves it) and read (passes whose leader waited, microseconds waited)."""
        w, us = C.c_uint64(0), C.c_uint64(0)
        _raise(self._L.vl_index_coalesce_gather(self._h, -1 if adaptive is None else int(bool(adaptive)), C.byref(w), C.byref(us)))
        return int(w.value), int(us.value)

    def graph(self, with_rows: bool = False) -> Dict[str, Any]:
        """The graph as it stands (vl_index_hnsw_graph_info / _export): entry, max_level, m, m0 and the arrays
        level[n], upper_off[n], cnt0[n], nbr0[n, m0], cntU[slots], nbrU[slots, m], node_ids[n], live[n] (+ rows[n, dim])."""
        n, slots = C.c_uint64(0), C.c_uint64(0)
        entry, m, m0 = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        lvl = C.c_int(0)
        _raise(self._L.vl_index_hnsw_graph_info(self._h, C.byref(n), C.byref(entry), C.byref(lvl), C.byref(m), C.byref(m0),
                                                C.byref(slots)))
        nn, ns, d = int(n.value), int(slots.value), self.dimension()
        g = {"entry": int(entry.value), "max_level": int(lvl.value), "m": int(m.value), "m0": int(m0.value), "n": nn,
             "level": np.zeros(max(nn, 1), np.uint8), "upper_off": np.zeros(max(nn, 1), np.uint32),
             "cnt0": np.zeros(max(nn, 1), np.uint32), "nbr0": np.zeros((max(nn, 1), int(m0.value)), np.uint32),
             "cntU": np.zeros(max(ns, 1), np.uint32), "nbrU": np.zeros((max(ns, 1), int(m.value)), np.uint32),
             "node_ids": np.zeros(max(nn, 1), np.uint64), "live": np.zeros(max(nn, 1), np.uint8)}
        rows = np.zeros((max(nn, 1), d), np.float64) if with_rows else None
        vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p()  # noqa: E731
        _raise(self._L.vl_index_hnsw_graph_export(self._h, vp(g["level"]), vp(g["upper_off"]), vp(g["cnt0"]), vp(g["nbr0"]),
                                                  vp(g["cntU"]), vp(g["nbrU"]), vp(g["node_ids"]), vp(g["live"]), vp(rows)))
        if with_rows:
            g["rows"] = rows[:nn]
        for key in ("level", "upper_off", "cnt0", "nbr0", "node_ids", "live"):
            g[key] = g[key][:nn]
        g["cntU"], g["nbrU"] = g["cntU"][:ns], g["nbrU"][:ns]
        return g

    def params(self) -> Dict[str, int]:
        """The four build parameters: {"m", "m0", "ef_construction", "seed"} (vl_index_hnsw_params)."""
        m, m0, efc, seed = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        _raise(self._L.vl_index_hnsw_params(self._h, C.byref(m), C.byref(m0), C.byref(efc), C.byref(seed)))
        return {"m": int(m.value), "m0": int(m0.value), "ef_construction": int(efc.value), "seed": int(seed.value)}

    _GRAPH_ARRAYS = (("cnt0", np.uint32, 1), ("nbr0", np.uint32, 2), ("cntU", np.uint32, 1), ("nbrU", np.uint32, 2),
                     ("node_ids", np.uint64, 1), ("live", np.uint8, 1), ("rows", np.float64, 2))

    def _import_graph(self, g) -> int:
        """vl_index_hnsw_graph_import of the dict graph(with_rows=True) returns into this (empty) index; returns the
        number of nodes without an incoming layer-0 edge.  Shapes, dtypes and -- where the dict carries them -- level[]
        and upper_off[] against the level law of this index's (seed, m) are checked here, the lists by the library."""
        p, dim = self.params(), self.dimension()
        for key in ("m", "m0") + tuple(k for k, _, _ in self._GRAPH_ARRAYS):
            if key not in g:
                raise IndexOpError(f"graph import: the graph has no '{key}'")
        if int(g["m"]) != p["m"] or int(g["m0"]) != p["m0"]:
            raise IndexOpError(f"graph import: the graph has m = {int(g['m'])}, m0 = {int(g['m0'])}, the index m = {p['m']}, m0 = {p['m0']}")
        a = {}
        for key, dtype, ndim in self._GRAPH_ARRAYS:
            x = np.asarray(g[key])
            if x.dtype != dtype or x.ndim != ndim:
                raise IndexOpError(f"graph import: '{key}' must be a {ndim}-d {np.dtype(dtype).name} array, got {x.ndim}-d {x.dtype.name}")
            a[key] = np.ascontiguousarray(x)
        n, ns = a["cnt0"].shape[0], a["cntU"].shape[0]
        if "n" in g and int(g["n"]) != n:
            raise IndexOpError(f"graph import: n = {int(g['n'])} but cnt0 holds {n} entries")
        want = {"nbr0": (n, p["m0"]), "nbrU": (ns, p["m"]), "node_ids": (n,), "live": (n,), "rows": (n, dim)}
        for key, shape in want.items():
            if a[key].shape != shape:
                raise IndexOpError(f"graph import: '{key}' has shape {a[key].shape}, expected {shape}")
        if "level" in g or "upper_off" in g:
            law = hnsw_levels(p["seed"], n, p["m"])
            off = np.cumsum(law, dtype=np.uint64) - law
            for key, ref in (("level", law), ("upper_off", off)):
                if key not in g:
                    continue
                x = np.asarray(g[key])
                if x.shape != (n,) or not np.array_equal(x.astype(np.uint64), ref.astype(np.uint64)):
                    raise IndexOpError(f"graph import: '{key}' is not the level law of seed {p['seed']}, m {p['m']}: "
                                       "the graph was exported from an index with another seed or m")
        vp = lambda x: C.c_void_p(x.ctypes.data) if x.size else C.c_void_p()  # noqa: E731
        orphans = C.c_uint64(0)
        rc = self._L.vl_index_hnsw_graph_import(self._h, n, vp(a["node_ids"]), vp(a["live"]), vp(a["rows"]), 0, vp(a["cnt0"]),
                                                vp(a["nbr0"]), ns, vp(a["cntU"]), vp(a["nbrU"]), C.byref(orphans))
        if rc in (VL_ERR_INVALID_ARG, VL_ERR_DUP_ID):
            raise IndexOpError(_last_error())
        _raise(rc)
        return int(orphans.value)

    def import_times(self) -> Dict[str, float]:
        """Milliseconds of the last import: host validation, row ingest, uploads, edge-key kernel, in-degree kernel."""
        ms = (C.c_double * 5)()
        _raise(self._L.vl_index_hnsw_import_times(self._h, ms))
        return dict(zip(("validate_ms", "ingest_ms", "upload_ms", "edge_key_kernel_ms", "indegree_kernel_ms"), (float(x) for x in ms)))

    @classmethod
    def from_graph(cls, g, dim: int, metric: int, device: int = 0, ef_construction: int = 400, seed: int = 0,
                   m: Optional[int] = None, m0: Optional[int] = None) -> "HNSWIndex":
        """An index from the dict graph(with_rows=True) returns, without rebuilding: the lists are taken as given, the
        levels follow from (seed, m), and what the dict does not carry is recomputed on the device.  m and m0 are read
        from the dict (if named they must agree); pass the exporter's params().  IndexOpError with the library's text
        for a list that breaks the graph's invariants, a duplicate live id or a graph of another seed.  _meta starts
        empty."""
        for key, given in (("m", m), ("m0", m0)):
            if key not in g:
                raise IndexOpError(f"graph import: the graph has no '{key}'")
            if given is not None and int(given) != int(g[key]):
                raise IndexOpError(f"graph import: {key} = {int(given)} was asked for, the graph has {int(g[key])}")
        idx = cls(dim, metric, device=device, m=int(g["m"]), m0=int(g["m0"]), ef_construction=ef_construction, seed=seed)
        idx._import_graph(g)
        return idx

    def save_snapshot(self, path: str) -> None:
        """The whole index -- graph, rows, tombstones, parameters and _meta -- as one .npz file (written under a
        temporary name and renamed).  load_snapshot() brings it back without rebuilding."""
        g, p = self.graph(with_rows=True), self.params()
        meta = json.dumps([[int(i), t, md] for i, (t, md) in self._meta.items()])
        tmp = f"{path}.tmp.{os.getpid()}"
        try:
            with open(tmp, "wb") as f:
                np.savez(f, format=np.array(self._SNAPSHOT_FORMAT), dim=np.uint64(self.dimension()), metric=np.int32(int(self.metric())),
                         m=np.uint32(p["m"]), m0=np.uint32(p["m0"]), ef_construction=np.uint32(p["ef_construction"]),
                         seed=np.uint64(p["seed"]), entry=np.uint32(g["entry"]), max_level=np.int32(g["max_level"]),
                         meta=np.array(meta), **{k: g[k] for k in self._SNAPSHOT_ARRAYS})
            os.replace(tmp, path)
        finally:
            if os.path.exists(tmp):
                os.unlink(tmp)

    _SNAPSHOT_FORMAT = "vectorlite-hnsw-snapshot-1"
    _SNAPSHOT_ARRAYS = ("level", "upper_off", "cnt0", "nbr0", "cntU", "nbrU", "node_ids", "live", "rows")

    @classmethod
    def load_snapshot(cls, path: str, device: int = 0) -> "HNSWIndex":
        """The index save_snapshot() wrote.  PersistenceError for a file that is missing, cut short, lacks a member, has
        a member of the wrong shape or type, or holds a list the import refuses."""
        from .persistence import FileNotFound, PersistenceError
        if not os.path.exists(path):
            raise FileNotFound(f"File not found: {path}")
        try:
            with np.load(path, allow_pickle=False) as z:
                if str(z["format"][()]) != cls._SNAPSHOT_FORMAT:
                    raise PersistenceError(f"Expected format '{cls._SNAPSHOT_FORMAT}', got '{z['format'][()]}'")
                s = {k: z[k][()] for k in ("dim", "metric", "m", "m0", "ef_construction", "seed", "entry", "max_level")}
                for k, v in s.items():
                    if np.ndim(v) != 0 or not np.issubdtype(np.asarray(v).dtype, np.integer):
                        raise PersistenceError(f"snapshot member '{k}' is not an integer scalar")
                g = {k: z[k] for k in cls._SNAPSHOT_ARRAYS}
                meta = json.loads(str(z["meta"][()]))
        except PersistenceError:
            raise
        except Exception as e:  # a cut-short or foreign file: zipfile, numpy and json each have their own error types
            raise PersistenceError(f"cannot read HNSW snapshot {path}: {type(e).__name__}: {e}") from e
        g["m"], g["m0"] = int(s["m"]), int(s["m0"])
        try:
            idx = cls.from_graph(g, int(s["dim"]), int(s["metric"]), device=device, ef_construction=int(s["ef_construction"]),
                                 seed=int(s["seed"]))
        except (IndexOpError, ValueError) as e:
            raise PersistenceError(f"HNSW snapshot {path} refused: {e}") from e
        got = idx.graph()
        if g["cnt0"].shape[0] and (got["entry"], got["max_level"]) != (int(s["entry"]), int(s["max_level"])):
            raise PersistenceError(f"HNSW snapshot {path} refused: entry / max_level do not follow from its levels")
        try:
            idx._meta = {int(i): (t, md) for i, t, md in meta}
        except Exception as e:
            raise PersistenceError(f"HNSW snapshot {path}: malformed meta: {e}") from e
        return idx

    def set_min_beam(self, min_beam: int) -> None:
        """Opt-in beam floor of searches that name no ef; default 0 = the reference's strict ef = min(k, len)."""
        _raise(self._L.vl_index_hnsw_set_min_beam(self._h, int(min_beam)))

    _NAVIGATION = {"f32": 0, "reference": 1}  # VL_HNSW_NAV_F32, VL_HNSW_NAV_REFERENCE

    def set_navigation(self, mode: str) -> None:
        """How walks navigate: "f32" (default; f32 steering, the final beam re-scored with the reference's u64) or
        "reference" (opt-in; every evaluation the reference's u64, ties in first-seen order: the CPU restatement of
        the published walk, oracle/vl_hnsw_cpu.c, node for node).  A clone starts in "f32"."""
        if not isinstance(mode, str) or mode not in self._NAVIGATION:
            raise ValueError(f"navigation mode must be 'f32' or 'reference', got {mode!r}")
        _raise(self._L.vl_index_hnsw_set_navigation(self._h, self._NAVIGATION[mode]))

    def walk_stats(self) -> Tuple[int, int]:
        """(queries walked, distance evaluations made for them) since creation."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _raise(self._L.vl_index_hnsw_walk_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def clone(self) -> "HNSWIndex":
        """Deep copy (rows + device graph, tombstones included): #[derive(Clone)] on HNSWIndex."""
        h = C.c_void_p()
        _raise(self._L.vl_index_clone(self._h, C.byref(h)))
        c = HNSWIndex(self.dimension(), device=self.device, _handle=h)
        c._meta = dict(self._meta)
        return c

    def export(self) -> Tuple[np.ndarray, np.ndarray]:
        """(ids, values) of the live rows in insertion order: the serialised `vector_values`."""
        n, d = self.len(), self.dimension()
        ids = np.empty(max(n, 1), dtype=np.uint64)
        vals = np.empty((max(n, 1), max(d, 1)), dtype=np.float64)
        _raise(self._L.vl_index_export(self._h, _pu64(ids), _pf64(vals)))
        return ids[:n].copy(), vals[:n, :d].copy()

    def metric(self) -> SimilarityMetric:
        m = C.c_int(0)
        _raise(self._L.vl_index_metric(self._h, C.byref(m)))
        return SimilarityMetric(m.value)

    def add(self, vector: Vector) -> None:
        vals = _f64(vector.values).ravel()
        rc = self._L.vl_index_add(self._h, int(vector.id), _pf64(vals), vals.size)
        if rc in (VL_ERR_DIM_MISMATCH, VL_ERR_DUP_ID):
            raise IndexOpError(_last_error())
        _raise(rc)
        self._meta[int(vector.id)] = (vector.text, vector.metadata)

    def add_rows(self, ids, values) -> None:
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64))
        on_device = False
        try:
            import torch
            is_tensor = isinstance(values, torch.Tensor)
        except Exception:  # pragma: no cover
            is_tensor = False
        if is_tensor and values.is_cuda:
            import torch
            if values.dtype != torch.float64 or not values.is_contiguous():
                raise ValueError("device rows must be a contiguous float64 tensor")
            torch.cuda.current_stream(values.device).synchronize()
            ptr, on_device = C.c_void_p(values.data_ptr()), True
            count = values.numel()
        else:
            vals = _f64(values.numpy() if is_tensor else values)
            ptr, count = C.c_void_p(vals.ctypes.data), vals.size
        if count != ids.size * self.dimension():
            raise ValueError("values must be [n, dim]")
        rc = self._L.vl_index_add_bulk(self._h, _pu64(ids), ptr, ids.size, 1, 1 if on_device else 0)
        if rc == VL_ERR_DUP_ID:
            raise IndexOpError(_last_error())
        _raise(rc)

    def add_embeddings(self, ids, embeddings, normalize: bool = True) -> None:
        """f32 model output -> normalised f64 rows on the device (src/embeddings.rs:169-181) -> n x add()."""
        _add_embeddings(self._L, self._h, self.dimension(), ids, embeddings, normalize, True)

    def delete(self, id: int) -> None:
        rc = self._L.vl_index_delete(self._h, int(id))
        if rc == VL_ERR_NOT_FOUND:
            raise IndexOpError(_last_error())  # "Vector ID {id} does not exist" (:401-403)
        _raise(rc)
        self._meta.pop(int(id), None)

    def delete_many(self, ids) -> int:
        """`for id in ids: delete(id)` under one lock (vl_index_delete_bulk): stops at the first id that does not exist and
        raises its error; the ids before it stay deleted.  Returns the nodes tombstoned."""
        arr = _u64_array(ids)
        removed = C.c_uint64(0)
        rc = self._L.vl_index_delete_bulk(self._h, _pu64(arr), arr.size, C.byref(removed))
        for i in arr[: int(removed.value)].tolist():
            self._meta.pop(i, None)
        if rc == VL_ERR_NOT_FOUND:
            raise IndexOpError(_last_error())  # "Vector ID {id} does not exist" (:401-403)
        _raise(rc)
        return int(removed.value)

    def update(self, vector: Vector) -> None:
        """Not served on HNSW handles (the graph's edge keys are distances of the old values): the library's error."""
        vals = _f64(vector.values).ravel()
        rc = self._L.vl_index_update(self._h, int(vector.id), _pf64(vals), vals.size)
        if rc in (VL_ERR_NOT_FOUND, VL_ERR_INVALID_ARG):
            raise IndexOpError(_last_error())
        _raise(rc)

    def update_rows(self, ids, values, insert_missing: bool = False) -> Tuple[int, int]:
        """Not served on HNSW handles: the library's error."""
        return _update_rows(self._L, self._h, self.dimension(), ids, values, insert_missing)

    def upsert_rows(self, ids, values) -> Tuple[int, int]:
        return self.update_rows(ids, values, insert_missing=True)

    def _raise_search(self, rc: int, requested: int):
        if rc == VL_ERR_METRIC_MISMATCH:
            raise MetricMismatch(SimilarityMetric(int(requested)), self.metric())
        _raise(rc)

    def search_batch(self, queries, k: int, metric: int, ef: int = 0, filter=None):
        """(ids [nq, k], scores [nq, k], n [nq]); ef = 0 is the reference's ef = min(k, len).  filter: a WalkFilter of
        this index or an iterable of ids (a temporary filter) -- one filter for every query of the batch."""
        Q = _f64(queries)
        if Q.ndim == 1:
            Q = Q[None, :]
        nq, qlen = Q.shape
        # buffers hold min(k, len) entries per query and k is clamped to them (a prefix of the same ranking): a huge k
        # costs nothing, and an add() from another thread after len() was read cannot make the library overrun them
        kk = max(min(int(k), self.len()), 1)
        kc = min(int(k), kk)
        ids = np.zeros((nq, kk), dtype=np.uint64)
        scores = np.zeros((nq, kk), dtype=np.float64)
        n = np.zeros(max(nq, 1), dtype=np.uint64)
        if filter is None:
            rc = self._L.vl_index_search_ef(self._h, _pf64(Q), nq, qlen, kc, int(ef), int(metric), _pu64(ids),
                                            _pf64(scores), _pu64(n))
        else:
            wf, temporary = self._walk_filter(filter)
            try:
                rc = self._L.vl_index_search_ef_filtered(self._h, wf.token, _pf64(Q), nq, qlen, kc, int(ef), int(metric), kk,
                                                         _pu64(ids), _pf64(scores), _pu64(n))
            finally:
                if temporary:
                    wf.close()
        self._raise_search(rc, metric)
        return ids[:, :kc], scores[:, :kc], n[:nq]

    def make_walk_filter(self, ids) -> WalkFilter:
        """A WalkFilter over `ids` (any iterable of ints; unsorted, repeats and ids the index does not hold are fine)."""
        ids = np.ascontiguousarray(np.fromiter((int(i) for i in ids), dtype=np.uint64)
                                   if not isinstance(ids, np.ndarray) else ids.astype(np.uint64, copy=False))
        tok, nodes = C.c_uint64(0), C.c_uint64(0)
        rc = self._L.vl_index_hnsw_filter_create(self._h, _pu64(ids), ids.size, C.byref(tok), C.byref(nodes))
        if rc == VL_ERR_INVALID_ARG:
            raise IndexOpError(_last_error())
        _raise(rc)
        return WalkFilter(self, int(tok.value))

    def _walk_filter(self, filter):
        """(WalkFilter, whether it is a temporary one the caller closes).  An IdFilter raises as make_filter does."""
        if isinstance(filter, WalkFilter):
            if filter._index is not self or not filter.token:
                raise IndexOpError("the filter is closed or belongs to another index")
            return filter, False
        if isinstance(filter, IdFilter):
            self.make_filter([])  # raises: flat filters do not serve HNSW handles
        return self.make_walk_filter(filter), True

    def last_filtered(self) -> Dict[str, int]:
        """The last filtered search on this index: route (0 walk, 1 exact), the walk's list capacity, the nodes that
        passed, and the walks in which the capacity dropped a list entry."""
        route, cap, nodes, cut = C.c_int(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        _raise(self._L.vl_index_hnsw_last_filtered(self._h, C.byref(route), C.byref(cap), C.byref(nodes), C.byref(cut)))
        return {"route": int(route.value), "cap": int(cap.value), "pass_nodes": int(nodes.value), "cap_cut_walks": int(cut.value)}

    def make_filter(self, ids, exclude: bool = False) -> IdFilter:
        """Filtered search is served by single-GPU flat indexes: raises IndexOpError with the library's message."""
        return _make_filter(self._L, self._h, self, ids, exclude)

    def search_range_arrays(self, query, min_score: float, metric: int = 0, filter=None, limit=None):
        """Range search is served by single-GPU flat indexes: raises IndexOpError with the library's message."""
        return _search_range(self._L, self._h, query, min_score, metric, 0, limit)

    def search_range(self, query, min_score: float, similarity_metric: int = SimilarityMetric.Cosine, filter=None, limit=None):
        return self.search_range_arrays(query, min_score, similarity_metric, filter, limit)

    def search_range_batch_arrays(self, queries, min_score, metric: int = 0, filter=None, limit=None):
        """Batched range search is served by single-GPU flat indexes: raises IndexOpError with the library's message."""
        return _search_range_batch(self._L, self._h, queries, min_score, metric, 0, limit)

    def search_range_batch(self, queries, min_score, similarity_metric: int = SimilarityMetric.Cosine, filter=None, limit=None):
        return self.search_range_batch_arrays(queries, min_score, similarity_metric, filter, limit)

    def search_mmr_arrays(self, query, k: int, fetch_k: int = 20, lambda_mult: float = 0.5, metric: int = 0, filter=None):
        """Diversified search is served by single-GPU flat indexes: raises IndexOpError with the library's message."""
        return _search_mmr(self._L, self._h, query, k, fetch_k, lambda_mult, metric, 0)

    def search_mmr(self, query, k: int, fetch_k: int = 20, lambda_mult: float = 0.5,
                   similarity_metric: int = SimilarityMetric.Cosine, filter=None):
        return self.search_mmr_arrays(query, k, fetch_k, lambda_mult, similarity_metric, filter)

    def search_mmr_batch_arrays(self, queries, k: int, fetch_k: int = 20, lambda_mult: float = 0.5, metric: int = 0, filter=None):
        """Diversified search is served by single-GPU flat indexes: raises IndexOpError with the library's message."""
        return _search_mmr_batch(self._L, self._h, queries, k, fetch_k, lambda_mult, metric, 0)

    def search_mmr_batch(self, queries, k: int, fetch_k: int = 20, lambda_mult: float = 0.5,
                         similarity_metric: int = SimilarityMetric.Cosine, filter=None):
        return self.search_mmr_batch_arrays(queries, k, fetch_k, lambda_mult, similarity_metric, filter)

    def make_groups(self, ids, keys) -> GroupTable:
        """Grouped search is served by single-GPU flat indexes: raises IndexOpError with the library's message."""
        return _make_groups(self._L, self._h, self, ids, keys)

    def make_attribute(self, ids, values) -> AttrColumn:
        """Attribute columns are served by single-GPU flat indexes: raises IndexOpError with the library's message."""
        return _make_attribute(self._L, self._h, self, ids, values)

    def make_filter_where(self, clauses) -> IdFilter:
        """Predicate filters are served by single-GPU flat indexes: raises IndexOpError with the library's message."""
        return _make_filter_where(self._L, self._h, self, clauses)

    def search_grouped_arrays(self, query, k: int, metric: int = 0, groups=None, filter=None):
        """Grouped search is served by single-GPU flat indexes: raises IndexOpError with the library's message."""
        self.make_groups([], [])  # raises: no grouped HNSW walk

    def search_grouped(self, query, k: int, similarity_metric: int = SimilarityMetric.Cosine, groups=None, filter=None):
        return self.search_grouped_arrays(query, k, similarity_metric, groups, filter)

    def search_grouped_batch_arrays(self, queries, k: int, metric: int = 0, groups=None, filter=None):
        """Grouped search is served by single-GPU flat indexes: raises IndexOpError with the library's message."""
        self.make_groups([], [])  # raises: no grouped HNSW walk

    def search_grouped_batch(self, queries, k: int, similarity_metric: int = SimilarityMetric.Cosine, groups=None, filter=None):
        return self.search_grouped_batch_arrays(queries, k, similarity_metric, groups, filter)

    def search_arrays(self, query, k: int, metric: int, ef: int = 0, filter=None, exclude=None):
        if exclude is not None:
            self.make_filter([], exclude=True)  # raises: exclusion filters do not serve HNSW handles
        ids, scores, n = self.search_batch(_f64(query).ravel()[None, :], k, metric, ef, filter=filter)
        m = int(n[0])
        return ids[0, :m].copy(), scores[0, :m].copy()

    def search(self, query, k: int, similarity_metric: int, filter=None, exclude=None) -> List[SearchResult]:
        if filter is not None or exclude is not None:
            ids, scores = self.search_arrays(query, k, similarity_metric, 0, filter, exclude)
            out = []
            for i, s in zip(ids.tolist(), scores.tolist()):
                text, md = self._meta.get(i, ("", None))
                out.append(SearchResult(id=i, score=s, text=text, metadata=md))
            return out
        q = _f64(query).ravel()
        kk = max(min(int(k), self.len()), 1)
        ids = np.zeros(kk, dtype=np.uint64)
        scores = np.zeros(kk, dtype=np.float64)
        n = C.c_uint64(0)
        rc = self._L.vl_index_search(self._h, _pf64(q), q.size, min(int(k), kk), int(similarity_metric), _pu64(ids),
                                     _pf64(scores), C.byref(n))
        self._raise_search(rc, similarity_metric)
        out = []
        for i, s in zip(ids[: n.value].tolist(), scores[: n.value].tolist()):
            text, md = self._meta.get(i, ("", None))
            out.append(SearchResult(id=i, score=s, text=text, metadata=md))
        return out

    def len(self) -> int:
        return int(self._L.vl_index_len(self._h))

    __len__ = len

    def is_empty(self) -> bool:
        return bool(self._L.vl_index_is_empty(self._h))

    def dimension(self) -> int:
        return int(self._L.vl_index_dimension(self._h))

    def get_vector(self, id: int) -> Optional[Vector]:
        out = np.empty(self.dimension(), dtype=np.float64)
        rc = self._L.vl_index_get_vector(self._h, int(id), _pf64(out))
        if rc == VL_ERR_NOT_FOUND:
            return None
        _raise(rc)
        text, md = self._meta.get(int(id), ("", None))
        return Vector(id=int(id), values=out.tolist(), text=text, metadata=md)

    def max_id(self) -> Optional[int]:
        out = C.c_uint64(0)
        rc = self._L.vl_index_max_id(self._h, C.byref(out))
        if rc == VL_ERR_NOT_FOUND:
            return None
        _raise(rc)
        return out.value
