/*
 * vectorlite_amd.h -- C ABI of the MI355X-native distance-scan engine.
 *
 * Drop-in boundary for ONE path of mmailhos/vectorlite v0.1.5: the distance
 * scan + top-k behind `trait VectorIndex` (src/lib.rs:224-245), i.e. what
 * `FlatIndex` (src/index/flat.rs:60-135) and the distance callbacks / score
 * post-processing of `HNSWIndex` (src/index/hnsw.rs:113-174, :415-496) do.
 * A Rust `impl VectorIndex for GpuFlatIndex` binds these symbols through
 * `extern "C"`; text/metadata stay on the Rust side keyed
 * by id -- this library returns (id, score) pairs only.
 *
 * Conventions
 *  - plain pointers and sizes only; the caller owns every in/out buffer and the
 *    library keeps no pointer past the call;
 *  - every function returns a vl_status; no C++ exception crosses the boundary;
 *  - vectors, queries and scores are f64 like the reference
 *    (src/lib.rs:168,198,232); ids are arbitrary u64;
 *  - search calls are re-entrant and may run concurrently from many threads on
 *    one handle (the reference searches under RwLock::read, src/client.rs:398);
 *    add/delete take the handle exclusively (RwLock::write, src/client.rs:333,383);
 *  - there is NO CPU fallback: without a usable HIP device every compute entry
 *    point returns VL_ERR_DEVICE.
 */
#ifndef VECTORLITE_AMD_H
#define VECTORLITE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* enum SimilarityMetric, declaration order (src/lib.rs:363-378) */
typedef enum vl_metric {
    VL_COSINE = 0,     /* cosine_similarity     src/lib.rs:425-444 */
    VL_EUCLIDEAN = 1,  /* euclidean_similarity  src/lib.rs:476-489 */
    VL_MANHATTAN = 2,  /* manhattan_similarity  src/lib.rs:521-532 */
    VL_DOTPRODUCT = 3  /* dot_product           src/lib.rs:565-572 */
} vl_metric;

typedef enum vl_status {
    VL_OK = 0,
    VL_ERR_DIM_MISMATCH = 1,    /* DimensionMismatch{expected,actual} src/errors.rs:18; "Vector dimension mismatch" src/index/flat.rs:84 */
    VL_ERR_DUP_ID = 2,          /* "Vector ID {} already exists"      src/index/flat.rs:87 */
    VL_ERR_NOT_FOUND = 3,       /* "Vector ID {} does not exist"      src/index/hnsw.rs:401-403; get_vector -> None */
    VL_ERR_METRIC_MISMATCH = 4, /* MetricMismatch{requested,index}    src/errors.rs:42, src/index/hnsw.rs:425-430 */
    VL_ERR_NAN_SCORE = 5,       /* stands in for the partial_cmp().unwrap() panic, src/index/flat.rs:116 */
    VL_ERR_DEVICE = 6,          /* HIP runtime / kernel failure, or no device */
    VL_ERR_OOM = 7,             /* host or device allocation failed */
    VL_ERR_INVALID_ARG = 8,     /* null pointer, unknown metric, ... */
    /* .vlc loader (PersistenceError, src/persistence.rs:34-54) */
    VL_ERR_IO = 9,               /* "IO error: {0}" */
    VL_ERR_FILE_NOT_FOUND = 10,  /* "File not found: {0}" */
    VL_ERR_SERIALIZATION = 11,   /* "Serialization error: {0}" (malformed JSON, missing field, bad row) */
    VL_ERR_VERSION_MISMATCH = 12,/* "Version mismatch: expected 1.0.0, got {actual}" */
    VL_ERR_INVALID_FORMAT = 13   /* "Invalid file format: Expected format 'vectorlite-collection', got '{}'" */
} vl_status;

/* Which search pipeline produced the last result on this thread (diagnostics). */
typedef enum vl_path {
    VL_PATH_NONE = 0,
    VL_PATH_FAST = 1,       /* f32 slab scan -> top-64 candidates -> exact f64 rescoring, bound check passed */
    VL_PATH_EXACT_SELECT = 2, /* full f64 scan in reference arithmetic + exact top-k select (k <= 64) */
    VL_PATH_EXACT_SORT = 3    /* full f64 scan + device-wide sort (any k) */
} vl_path;

typedef struct vl_index vl_index; /* opaque; Send + Sync */

/* ---- lifecycle ---------------------------------------------------------- */

/* FlatIndex::new(dim, Vec::new())  (src/index/flat.rs:68-73) on HIP device `device`. */
int vl_flat_create(uint64_t dim, int device, vl_index **out);

/* FlatIndex::new(dim, data) with n rows: like the reference it validates
 * nothing (duplicate ids are kept).  `values` is [n, dim] row-major f64 on the host. */
int vl_flat_from_rows(uint64_t dim, const uint64_t *ids, const double *values, uint64_t n, int device,
                      vl_index **out);

/* ONE flat index over several GPUs of the node, in ONE process (the reference is one process: collections live in
 * Arc<RwLock<..>>, src/client.rs:243-247; searches run under read() on any tokio worker, src/client.rs:398,
 * src/server.rs:269,379-392).  The handle answers every vl_index_* entry point like a vl_flat_create handle
 * (VectorIndexWrapper::Flat); no per-GPU process, no id handshake.  device_ids[n_dev]: HIP ordinals, one part each
 * (an ordinal listed twice makes two parts on that card).
 *   VL_MULTI_REPLICAS    every GPU holds every row; add / delete go to all of them; a vl_index_search is answered by
 *                        the replica with the fewest searches in flight, on the calling thread (concurrent callers
 *                        spread over the GPUs; vl_index_set_coalescing gives each replica its own queue); a
 *                        vl_index_search_batch is cut into one run of queries per replica.
 *   VL_MULTI_ROW_SHARDS  every GPU holds part of the rows (add appends to the shortest shard; bulk adds are cut into
 *                        contiguous runs that level the shards).  Every search runs on all shards side by side, the
 *                        per-shard exact top-k are merged on the first GPU by (score desc, insertion order asc): the
 *                        answer is bit-identical to one index holding every row (src/index/flat.rs:116).
 * Device-side inputs (values_on_device, embeddings_on_device, d_queries) are expected on device_ids[0].
 * vl_index_search_positions returns global insertion numbers for a row-sharded handle. */
#define VL_MULTI_REPLICAS 0
#define VL_MULTI_ROW_SHARDS 1
int vl_flat_create_multi(uint64_t dim, const int *device_ids, int n_dev, int mode, vl_index **out);

/* Parts of a handle (1 for a single-GPU handle, mode -1): rows held by each part and searches each has answered
 * (queries, for batches) -- how evenly the replica dealer / the shard filler spread the work.  rows / searches hold
 * `capacity` entries and are filled when capacity >= *n_parts; any pointer may be NULL. */
int vl_index_parts(const vl_index *h, int *n_parts, int *mode, uint64_t *rows, uint64_t *searches, int capacity);

/* HNSWIndex::new(dim, metric) (src/index/hnsw.rs:216-259), default cargo profile M = 16, M0 = 32
 * (src/index/hnsw.rs:95-109).  The handle then behaves like VectorIndexWrapper::HNSW
 * (src/lib.rs:271-327) under every vl_index_* trait entry point below: add validates dimension and
 * duplicate ids (:363-371), delete of an absent id is VL_ERR_NOT_FOUND (:401-403) and tombstones the
 * node (:405-411), search checks the dimension even when empty (:416-421), rejects another metric with
 * VL_ERR_METRIC_MISMATCH (:425-430), walks the graph with ef = min(k, len) (:437,454), converts
 * u64 distances to scores (:51-75, :478-479), stable-sorts and truncates (:493-494).
 * The graph walk itself is this library's own (crate hnsw 0.11.0 is not part of the reference tree): it
 * navigates by f32 distances and gives every node of the final beam the reference's exact f64 callback value,
 * from which the returned scores are computed; results are approximate and judged by recall.
 * vl_hnsw_create builds with ef_construction = 400 -- what crate hnsw 0.11.0's Params::default() is recalled to be (the
 * reference passes no parameters, src/index/hnsw.rs:226-244; the crate is not in the reference tree, so unverified);
 * vl_hnsw_create_ex takes M, M0 (<= 64), ef_construction (1..512) and the level seed. */
int vl_hnsw_create(uint64_t dim, int metric, int device, vl_index **out);
int vl_hnsw_create_ex(uint64_t dim, int metric, uint32_t m, uint32_t m0, uint32_t ef_construction, uint64_t seed,
                      int device, vl_index **out);

/* #[derive(Clone)] (src/index/flat.rs:59, src/index/hnsw.rs:197; persistence clones the wrapper,
 * src/persistence.rs:118).  Flat: rows copied device to device.  HNSW: rows and the device graph are
 * copied as they are (tombstoned nodes included), so the clone answers exactly like the original. */
int vl_index_clone(const vl_index *h, vl_index **out);

void vl_index_destroy(vl_index *h);

/* Pre-size device storage for `n_rows` (optional; storage grows geometrically otherwise). */
int vl_index_reserve(vl_index *h, uint64_t n_rows);

/* ---- trait VectorIndex (src/lib.rs:224-245) ------------------------------- */

/* add(Vector): VL_ERR_DIM_MISMATCH if len != dim, VL_ERR_DUP_ID if id exists (src/index/flat.rs:82-91). */
int vl_index_add(vl_index *h, uint64_t id, const double *values, uint64_t len);

/* n x add() in order, one device pass.  validate != 0: stop at the first row whose id
 * already exists (rows before it are kept, like n sequential adds) and return VL_ERR_DUP_ID;
 * validate == 0: FlatIndex::new semantics (no checks).  values_on_device != 0: `values`
 * is a device pointer on the index's device ([n, dim] f64). */
int vl_index_add_bulk(vl_index *h, const uint64_t *ids, const double *values, uint64_t n, int validate,
                      int values_on_device);

/* NEW -- the ingest step in front of add (src/embeddings.rs:169-181): `embeddings` is [n, dim] f32 as the model
 * emits it (host pointer, or a device pointer on the index's device when embeddings_on_device != 0).  Each value
 * is widened to f64 (`x as f64`, :172) and, with normalize != 0, the row is L2-normalised on the device with the
 * host's arithmetic (:175-179: norm = sqrt of the in-order sum of squares; x / norm when norm > 0, else the row
 * unchanged), bit for bit.  The rows are then appended like vl_index_add_bulk (same `validate` meaning and
 * duplicate-id behaviour; HNSW handles always validate).  PCIe carries 4 bytes per value instead of 8. */
int vl_index_add_embeddings_f32(vl_index *h, const uint64_t *ids, const float *embeddings, uint64_t n, int normalize,
                                int validate, int embeddings_on_device);

/* delete(id): removes every row with that id, order-preserving; VL_OK even when
 * the id is absent (src/index/flat.rs:93-96). */
int vl_index_delete(vl_index *h, uint64_t id);

/* NEW capability: n deletes in one call.  The index is left in exactly the state `for (i < n_ids) vl_index_delete(h, ids[i])`
 * leaves it in -- length, row order, exported ids and f64 bits, every later search, filter, group table and clone -- but the
 * flat index finds the rows with one walk over its ids and compacts each device array in one pass (a row-move kernel over
 * the plan of DESIGN.md section 22), however many ids go, where n single deletes move the rows behind each id in turn.
 * Flat (also over several GPUs): absent ids are Ok, a repeated id is a no-op the second time, every row an id has goes;
 * always VL_OK short of a device error; *out_removed (may be null) = rows removed.  HNSW: the loop of tombstones under one
 * lock; stops at the first id that does not exist with VL_ERR_NOT_FOUND ("Vector ID {id} does not exist"), the ids before
 * it stay deleted (vl_index_add_bulk's prefix rule); *out_removed = nodes tombstoned. */
int vl_index_delete_bulk(vl_index *h, const uint64_t *ids, uint64_t n_ids, uint64_t *out_removed);

/* Bytes of the buffer a flat index's deletes compact through (it holds what a launch cannot move in place); 0 = the default
 * of 64 MB; never less than one row.  An existing smaller buffer is freed.  Diagnostic: small values make small indexes
 * exercise every kind of segment of the bulk delete's plan.  No effect on HNSW handles. */
int vl_index_set_delete_bounce(vl_index *h, uint64_t bytes);

/* Diagnostic (single-GPU flat handles): the last vl_index_delete_bulk (all zero if it removed nothing).  out6 = rows removed, rows moved
 * (those behind the first hole that stayed), launches that moved a segment in place, segments that went through the
 * bounce buffer, bytes written to device memory, microseconds from the first launch to the end of the synchronisation. */
int vl_index_last_delete(const vl_index *h, uint64_t *out6);

/* NEW capability (single-GPU flat handles): replace the values of a stored row in place.  update(id, v) rewrites the FIRST row
 * carrying `id` (vl_index_get_vector's rule; afterwards get_vector(id) returns v bit for bit) and, on the device, every copy
 * derived from it that exists for the row.  Length, row order, every other row, the ids, every filter / exclusion / group
 * token and its resolved state, and clones made earlier stay as they are; where delete + add would move the row to the end
 * and compact everything behind it, nothing moves.  Afterwards the handle answers every entry point as a flat index built
 * from the same (id, values) list in the same order.  VL_ERR_DIM_MISMATCH if len != dim, VL_ERR_NOT_FOUND ("Vector ID {id}
 * does not exist") if no row carries the id, VL_ERR_INVALID_ARG (the message says which) on HNSW and multi-GPU handles. */
int vl_index_update(vl_index *h, uint64_t id, const double *values, uint64_t len);

/* n updates in one call; `values` is [n, dim] f64 on the host.  The index is left in exactly the state of the loop
 * `for (i < n) contains(ids[i]) ? update(ids[i], values_i) : (insert_missing ? add(ids[i], values_i) : fail)`: a repeated id
 * keeps its last values; with insert_missing != 0 an absent id is appended once (where its first occurrence falls among the
 * appended rows, holding its last values) through the add path.  All or nothing: VL_ERR_NOT_FOUND (an absent id with
 * insert_missing == 0; "Vector ID {id} does not exist") and VL_ERR_INVALID_ARG (null pointers with n > 0; HNSW and
 * multi-GPU handles) are decided before any device write, and then nothing has changed.  n == 0 is VL_OK.  *out_updated =
 * distinct rows rewritten, *out_inserted = rows appended (either may be null).  DESIGN.md section 25. */
int vl_index_update_bulk(vl_index *h, const uint64_t *ids, const double *values, uint64_t n, int insert_missing,
                         uint64_t *out_updated, uint64_t *out_inserted);

/* Diagnostic (single-GPU flat handles): the last vl_index_update / vl_index_update_bulk (all zero if it did nothing).  out7 =
 * rows rewritten, rows appended, rows rewritten in the row-major bf16 copy, in the fragment-major bf16 copy, in the int8
 * copy, staging chunks, microseconds from the first launch to the end of the synchronisation. */
int vl_index_last_update(const vl_index *h, uint64_t *out7);

/* search(query, k, metric) (src/index/flat.rs:98-119): writes min(k, len) results, best first,
 * ties in insertion order.  out_ids/out_scores must hold min(k, len) entries; a caller that sized its
 * buffers from an earlier vl_index_len() passes k = min(k, capacity) -- results for a smaller k are a prefix
 * of those for a larger k, so the call can never write past the buffer even if the index grew since.
 * Empty index: any q_len is accepted and *out_n = 0.  Otherwise q_len != dim ->
 * VL_ERR_DIM_MISMATCH (vl_last_dim_mismatch gives expected/actual). */
int vl_index_search(const vl_index *h, const double *query, uint64_t q_len, uint64_t k, int metric,
                    uint64_t *out_ids, double *out_scores, uint64_t *out_n);

/* vl_index_search with an explicit output capacity: writes min(k, len, out_capacity) results -- the first
 * out_capacity entries of what vl_index_search would write (`truncate(k)`, src/index/flat.rs:117, applied once
 * more).  On an HNSW handle the walk still runs with the caller's k (its beam is ef = min(k, len),
 * src/index/hnsw.rs:437): only the copy-out is capped, so the entries ARE that prefix.  A caller that sized its buffers from an earlier vl_index_len() cannot be overrun by a concurrent add():
 * the bound is the caller's own number, not the index's length at search time.  The Rust / Python / C bindings of
 * this repository all call this form. */
int vl_index_search_cap(const vl_index *h, const double *query, uint64_t q_len, uint64_t k, int metric,
                        uint64_t out_capacity, uint64_t *out_ids, double *out_scores, uint64_t *out_n);

/* NEW capability (the reference has no batch entry, src/lib.rs:224-245): nq independent
 * searches, each with exactly vl_index_search's result.  queries is [nq, q_len];
 * out_ids/out_scores are [nq, k] (row stride k), out_n is [nq]. */
int vl_index_search_batch(const vl_index *h, const double *queries, uint64_t nq, uint64_t q_len, uint64_t k,
                          int metric, uint64_t *out_ids, double *out_scores, uint64_t *out_n);

/* The batch form with an explicit row capacity: out_ids / out_scores are [nq, out_stride]; row i receives
 * min(k, len, out_stride) entries, out_n[i] says how many (HNSW: the first out_stride entries of the walk with the
 * caller's k, as above). */
int vl_index_search_batch_cap(const vl_index *h, const double *queries, uint64_t nq, uint64_t q_len, uint64_t k,
                              int metric, uint64_t out_stride, uint64_t *out_ids, double *out_scores, uint64_t *out_n);

/* NEW capability (the reference restricts nothing): search among the rows whose id is in a set -- "documents of this
 * user", "chunks of this file", "rows whose metadata matches".  A filtered search returns exactly, ids and f64 scores,
 * what FlatIndex::search (src/index/flat.rs:98-119) returns on a FlatIndex holding ONLY the rows of h whose id is in the
 * set, in their storage order: ranking (score desc, insertion position asc) over the subset, every row whose id is in the
 * set qualifies (duplicate-id rows included), ids the index does not hold are ignored.  VL_ERR_NAN_SCORE only when a
 * subset row scores NaN (a lone qualifying row is returned whatever its score).  Errors are the unfiltered search's on
 * the WHOLE index: the dimension check runs whenever len(h) != 0 (an empty subset included), an unknown metric is
 * VL_ERR_INVALID_ARG, an empty subset or k = 0 gives *out_n = 0.
 * Single-GPU flat handles only: HNSW and vl_flat_create_multi handles return VL_ERR_INVALID_ARG.  Filtered calls never
 * join a coalesced pass.
 *
 * vl_index_filter_create: ids [n_ids] in any order, repeats allowed -> *out_filter, a token of this handle (never 0, never
 * reused); *out_rows (may be NULL) = rows that qualify now.  A filter follows the index: after add / delete the next use
 * resolves it again against the current rows.  vl_index_clone does not copy filters; vl_index_destroy frees them.
 * vl_index_filter_rows: rows that qualify now (resolving again if rows changed).
 * vl_index_filter_destroy: frees the token (a search using it at that moment finishes normally).
 * An unknown or destroyed token is VL_ERR_INVALID_ARG. */
int vl_index_filter_create(vl_index *h, const uint64_t *ids, uint64_t n_ids, uint64_t *out_filter, uint64_t *out_rows);
/* The opposite question -- "the best k, EXCEPT these ids" (rows already seen, the query document itself, soft-deleted rows):
 * a token of the same token space (never 0, never reused, not cloned, freed by vl_index_filter_destroy / vl_index_destroy,
 * resolved again on the first use after any add or delete) under which a row qualifies iff its id is NOT in the set.  ids in
 * any order, repeats allowed; n_ids = 0 keeps every row; an id the index does not hold is ignored until a row with that id is
 * added, which is then excluded; every row carrying an excluded id is excluded.  *out_rows and vl_index_filter_rows = len -
 * excluded rows.  Every flat entry point that takes a filter token takes this one, with its semantics read over "the
 * FlatIndex holding only the qualifying rows in storage order" (vl_index_search_batch_filters may mix both kinds); errors
 * are the include filter's, VL_ERR_NAN_SCORE only when a QUALIFYING row scores NaN.  The token costs a bitmap of len / 8
 * bytes; a single vl_index_search_filtered streams the unfiltered search's ladder (int8 / bf16 / f32 copies) under that
 * bitmap, the other calls build the position list (4 bytes per qualifying row) on first use.  DESIGN.md section 23. */
int vl_index_filter_create_excluding(vl_index *h, const uint64_t *ids, uint64_t n_ids, uint64_t *out_filter, uint64_t *out_rows);
int vl_index_filter_rows(const vl_index *h, uint64_t filter, uint64_t *out_rows);
int vl_index_filter_destroy(vl_index *h, uint64_t filter);

/* NEW capability: filters by VALUE instead of by id list -- "newer than t", "tenant = 17", "price in [a, b]" -- resolved on
 * the device, so a bound that changes per request costs one streaming pass over 8 bytes per row and column instead of a
 * host sort and an upload of the passing ids.  DESIGN.md section 28.
 * An ATTRIBUTE COLUMN maps ids to int64 values.  vl_index_attr_create: ids / values [n] in any order; a pair repeated exactly
 * is fine, an id given two different values within one call is VL_ERR_INVALID_ARG (the message names the smallest such id;
 * checked on the host before any device is touched), as are 2^32 - 1 pairs or more.  An id the index does not hold waits for
 * a row with that id to be added; a row whose id the column does not hold HAS NO VALUE; duplicate-id rows all get their
 * id's value.  *out_attr is a token of this handle from the filters' counter (never 0, never reused, not cloned, freed by
 * vl_index_attr_destroy / vl_index_destroy); *out_rows (may be NULL) and vl_index_attr_rows = rows that have a value now.
 * vl_index_attr_set upserts pairs: an id already held takes the new value, other ids are added, the same conflict rule
 * within the call; a refused call leaves the column as it was.  It waits for running searches, like add and delete.
 * Destroying a column leaves filter tokens made from it working; its memory goes with the last of them.
 * A column costs 16 bytes per pair on host and device, and 8 bytes + 1 bit per ROW of the index on the device. */
int vl_index_attr_create(vl_index *h, const uint64_t *ids, const int64_t *values, uint64_t n, uint64_t *out_attr,
                         uint64_t *out_rows);
int vl_index_attr_set(vl_index *h, uint64_t attr, const uint64_t *ids, const int64_t *values, uint64_t n);
int vl_index_attr_rows(const vl_index *h, uint64_t attr, uint64_t *out_rows);
int vl_index_attr_destroy(vl_index *h, uint64_t attr);
/* A PREDICATE filter token: 1 to 4 clauses, ANDed.  A row qualifies iff, for every clause, it has a value v in that column
 * and (lo <= v && v <= hi) != negate, compared as signed integers.  A row without a value never qualifies, even under
 * negate; lo > hi is legal (it keeps nothing, or with negate every row that has a value); equality is lo == hi.  A clause
 * count outside 1..4, reserved != 0, negate > 1 or an unknown column: VL_ERR_INVALID_ARG with a message.
 * The token belongs to the filter token space: vl_index_filter_rows / vl_index_filter_destroy work on it, and every flat
 * entry point that takes a filter token takes it, with the include token's semantics over "the FlatIndex holding only the
 * qualifying rows in storage order" and the include token's errors (vl_index_search_batch_filters may mix all three kinds).
 * It is resolved again on the first use after an add or delete or after vl_index_attr_set on one of its columns (the
 * columns first, then the predicate).  It costs len / 8 bytes (the keep bitmap) plus 4 bytes per qualifying row once a call
 * needs the position list; batches treat it as an exclusion token. */
typedef struct {
    uint64_t attr;
    int64_t lo;
    int64_t hi;
    uint32_t negate;
    uint32_t reserved;
} vl_where_clause;
int vl_index_filter_create_where(vl_index *h, const vl_where_clause *clauses, uint64_t n_clauses, uint64_t *out_filter,
                                 uint64_t *out_rows);
/* How a single vl_index_search_filtered under a predicate token runs.  0 (auto, the default; a clone keeps its source's
 * mode): the masked int8 / bf16 / f32 ladder when len x (bytes per row of the ladder's first stage) is strictly below
 * rows kept x the f32 row's bytes, else the position list -- near 25 % kept when the int8 copy goes first, near 50 % under
 * bf16, never when f32 goes first.  1: always the list.  2: the ladder wherever its conditions hold (no forced path, no row
 * outside the f32 domain, a stride the masked scan is compiled for, min(k, rows kept) <= 60), as exclusion tokens do.  The
 * answers are the same bits in every mode.  Flat single-GPU handles; others and a mode outside 0..2: VL_ERR_INVALID_ARG. */
int vl_index_set_where_route(vl_index *h, int mode);
/* out4[0] = the route of the last single predicate-filtered search on this handle (0 list, 1 masked ladder), [1] = the rows
 * its token kept, [2] = predicate resolutions, [3] = column resolutions on this handle so far. */
int vl_index_last_where(const vl_index *h, uint64_t *out4);

/* The filtered search, vl_index_search_cap's capacity rule: min(k, rows in the subset, out_capacity) entries, the prefix
 * of the k results. */
int vl_index_search_filtered(const vl_index *h, uint64_t filter, const double *query, uint64_t q_len, uint64_t k,
                             int metric, uint64_t out_capacity, uint64_t *out_ids, double *out_scores, uint64_t *out_n);

/* nq filtered searches with one filter, vl_index_search_batch_cap's layout: row i ([nq, out_stride]) is exactly
 * vl_index_search_filtered's answer for queries[i]. */
int vl_index_search_batch_filtered(const vl_index *h, uint64_t filter, const double *queries, uint64_t nq, uint64_t q_len,
                                   uint64_t k, int metric, uint64_t out_stride, uint64_t *out_ids, double *out_scores,
                                   uint64_t *out_n);

/* nq filtered searches, each with its own filter -- a server's batch of requests from different users.
 * row i = vl_index_search_filtered(h, filters[n_filters == 1 ? 0 : i], queries + i*q_len, q_len, k, metric, ...)
 * n_filters is 1 (one filter for the batch: vl_index_search_batch_filtered) or nq (one per query); rows out_stride apart,
 * capped at out_stride.  The same token may appear many times, filters may overlap, be empty or stale (every distinct
 * stale filter is resolved once per call).  The jobs share scan launches: one launch, one finalize and one
 * synchronisation for up to 512 (query, filter) pairs, the keys and the certificate of the single filtered search.
 * Checks are the single call's in its order: n_filters other than 1 or nq is VL_ERR_INVALID_ARG; then every token of the
 * array (0, unknown, destroyed: VL_ERR_INVALID_ARG); the metric; the dimension whenever len(h) != 0; k = 0 or nq = 0
 * is VL_OK with nothing written.  If a query fails (a NaN score inside its subset) the call returns the status of the
 * lowest-numbered failing query; rows in front of it hold their answers and out_n is 0 from that query on. */
int vl_index_search_batch_filters(const vl_index *h, const uint64_t *filters, uint64_t n_filters,
                                  const double *queries, uint64_t nq, uint64_t q_len, uint64_t k, int metric,
                                  uint64_t out_stride, uint64_t *out_ids, double *out_scores, uint64_t *out_n);
/* Of the last such call on this handle (either entry point; any argument may be NULL): batched = jobs answered by a
 * batched launch; single = jobs handed to the single filtered search before any launch (k beyond the fast path, a forced
 * path, a query or rows outside the f32 domain, a job alone in its launch); exact = jobs a batched launch could not
 * certify (redone on the exact kernels); launches = batched scan launches.  Jobs with an empty subset count nowhere. */
int vl_index_last_filtered_batch(const vl_index *h, uint64_t *batched, uint64_t *single, uint64_t *exact,
                                 uint64_t *launches);
/* How the two calls above answer queries under EXCLUSION tokens (vl_index_filter_create_excluding).  mode 0: with the
 * jobs launches, like include tokens.  1: every eligible query with the mask-aware MFMA batch pass -- one pass over the
 * bf16 rows per launch sequence whatever the number of queries, each query reading its own token's keep bitmap; no
 * position list is built for a token whose queries are all answered there.  2 (what new handles start in; a clone keeps
 * its source's mode): the pass when its estimated time is below the jobs launches'.  A query is eligible when the handle
 * has no forced path and no row outside the f32 domain, the metric is cosine, dot or Euclidean with a row length the MFMA
 * filter has a shape for, the index holds at least 8192 rows, min(k, rows kept) <= 60, at least one row is kept, and the
 * call holds at least two such queries.  The answers are the same bits in every mode: a query the pass cannot certify
 * joins the jobs like any other.  Flat single-GPU handles; others: VL_ERR_INVALID_ARG, as is a mode outside 0..2. */
int vl_index_set_masked_batch(vl_index *h, int mode);
/* Of the last vl_index_search_batch_filters / _filtered on this handle (any argument may be NULL): routed = queries sent
 * to the mask-aware pass; certified = those it answered; redone = those it handed back (counted by
 * vl_index_last_filtered_batch like any other job; queries answered by the pass are counted in none of its numbers);
 * sequences = launch sequences of the pass; lists_built = position lists of exclusion tokens the call had to build (0
 * when the pass answered every query of those tokens). */
int vl_index_last_masked_batch(const vl_index *h, uint64_t *routed, uint64_t *certified, uint64_t *redone,
                               uint64_t *sequences, uint64_t *lists_built);

/* NEW capability (the reference only answers "the best k"): every row that is at least this similar.  min_score is a
 * score in the reference's sense (higher is better for all four metrics, src/lib.rs:425-572; Euclidean and Manhattan are
 * 1 / (1 + d)).  The answer is the LONGEST PREFIX of FlatIndex::search(q, len, metric) (src/index/flat.rs:98-119) whose
 * scores satisfy the IEEE comparison score >= min_score, ids and f64 scores bit for bit: order (score desc, storage
 * position asc), rows that tie with the threshold are in, duplicate-id rows all count.  filter != 0 (a token of
 * vl_index_filter_create): "the index" is the FlatIndex holding only the filter's rows in storage order; 0 = whole index.
 * *out_total = rows that qualify, always; min(total, out_capacity) entries are written, the prefix of that ranking
 * (vl_index_search_cap's rule), *out_n of them.  out_capacity = 0 with NULL outputs is a legal "count only" call.
 * min_score = -inf returns the whole ranking; +inf, or anything above the best score, returns nothing with VL_OK; NaN is
 * VL_ERR_INVALID_ARG.  Errors are vl_index_search's on the same handle and query (dimension check whenever len != 0,
 * unknown metric); VL_ERR_NAN_SCORE exactly when search(q, len, metric) on the same (sub)index would return it.
 * Single-GPU flat handles only: HNSW and vl_flat_create_multi handles return VL_ERR_INVALID_ARG.  Range calls never
 * join a coalesced pass and read the f32 slab (no bf16 / int8 stage).  Other searches may run concurrently; add / delete
 * exclude it through the handle's reader/writer lock.  vl_last_path: VL_PATH_FAST, or VL_PATH_EXACT_SORT when more rows
 * pass the key-space threshold than the candidate buffer holds (2^20), data or query lie outside the fast-path domain,
 * or a path is forced. */
int vl_index_search_range(const vl_index *h, uint64_t filter, const double *query, uint64_t q_len, double min_score,
                          int metric, uint64_t *out_ids, double *out_scores, uint64_t out_capacity, uint64_t *out_n,
                          uint64_t *out_total);

/* nq range searches against ONE index state (one hold of the reader lock): near-duplicate detection asks every row of a
 * corpus, or a day's new rows, with one threshold.  Row i of the [nq, out_stride] outputs, out_n[i] and out_total[i] are
 * exactly what vl_index_search_range(h, filter, queries + i * q_len, q_len, min_scores[i], metric, ..., out_capacity =
 * out_stride, ...) returns on that state: ids, f64 score bits, counts -- so threshold ties are in, equal scores come in
 * storage order, -inf / +inf thresholds and duplicate ids behave as there.  out_stride = 0 with NULL id / score outputs
 * counts only.  nq = 0 is VL_OK and writes nothing.  The call returns the status the LOWEST-INDEX failing query's single
 * call would return (dimension check, unknown metric, a NaN min_scores[i] -> VL_ERR_INVALID_ARG, VL_ERR_NAN_SCORE exactly
 * when that query's single call returns it); outputs are unspecified on error.  HNSW and vl_flat_create_multi handles
 * return VL_ERR_INVALID_ARG.  Never joins a coalesced pass.
 * Route: with filter = 0, two or more queries, cosine / Euclidean / dot, a row length the batch filter has a shape for
 * (up to 768), in-domain rows and no forced path, one bf16 MFMA pass with per-query key thresholds derived from
 * min_scores[i] serves every query of a launch sequence, and rescore (the reference's f64 order), cut, rank and emit run on
 * the device.  A query outside the fast-path domain, a -inf threshold, a zero query under cosine, a query whose candidate
 * buffer (4096 rows) overflows or with more than 2048 qualifying rows is answered by the single call under the same lock.
 * Everything else (Manhattan, other row lengths, one query, filter != 0) is a loop over the single call under the lock. */
int vl_index_search_range_batch(const vl_index *h, uint64_t filter, const double *queries, uint64_t nq, uint64_t q_len,
                                const double *min_scores /* [nq] */, int metric, uint64_t out_stride,
                                uint64_t *out_ids, double *out_scores /* [nq, out_stride] */,
                                uint64_t *out_n, uint64_t *out_total /* [nq] */);

/* Diagnostics of the last successful vl_index_search_range_batch on this handle: how many of its queries were answered by
 * the MFMA pass with the device tail, by the single-query fast route (k_scan_range), and by the exact route
 * (VL_PATH_EXACT_SORT); the three sum to nq.  Any pointer may be NULL.  Single-GPU flat handles only. */
int vl_index_last_range_batch(const vl_index *h, uint64_t *mfma_queries, uint64_t *single_queries, uint64_t *exact_queries);
/* ... and the largest number of candidates the MFMA pass kept for one query it answered (0: none). */
int vl_index_last_range_batch_candidates(const vl_index *h, uint64_t *max_candidates);

/* NEW capability (the reference only answers "the best k"): k results that are relevant but not k copies of the same
 * paragraph -- maximal marginal relevance (MMR) over the exact candidates of a search.
 * Candidates: C = FlatIndex::search(query, fetch_k, metric) (src/index/flat.rs:98-119) on the whole index (filter = 0) or on
 * the FlatIndex of a filter's rows (a token of vl_index_filter_create), n = min(fetch_k, rows) of them in that ranking;
 * rel[i] = candidate i's score, row[i] its stored f64 row.  Candidates are rows: duplicate-id rows are distinct candidates.
 * Selection, every operation an IEEE f64 operation rounded on its own (nothing contracted into an FMA):
 *     one_minus = 1.0 - lambda;  sel = [0];  red[i] = -inf
 *     while len(sel) < min(k, n):
 *         j = sel[-1]
 *         for every i not in sel:  s = calculate(metric, row[i], row[j]) (src/lib.rs:380-391);  if s > red[i]: red[i] = s
 *         best = none
 *         for i = 0 .. n-1 not in sel, ascending:
 *             v = (lambda * rel[i]) - (one_minus * red[i]);  if best is none or v > v_best: best, v_best = i, v
 *         sel.append(best)
 * A NaN s never replaces red[i]; ties keep the better-ranked candidate; a NaN v never beats a standing best.
 * Output: min(k, n, out_capacity) entries, *out_n of them: entry t = (id, rel) of candidate sel[t], the reference score
 * bits, in SELECTION order (not sorted by score).  For fixed fetch_k and lambda the answer for a smaller k is a prefix of the
 * answer for a larger one (out_capacity: vl_index_search_cap's rule); lambda = 1 returns the first min(k, n) results of
 * search(query, fetch_k).
 * Errors: vl_index_search's on the same handle, query and fetch_k (dimension check whenever len != 0, unknown metric;
 * VL_ERR_NAN_SCORE exactly when search(query, fetch_k, metric) on the same (sub)index returns it).  lambda NaN or outside
 * [0, 1], fetch_k < k, fetch_k > VL_MMR_MAX_FETCH, an unknown or destroyed filter: VL_ERR_INVALID_ARG (checked before any
 * device is touched).  k = 0 or an empty (sub)index: *out_n = 0, VL_OK.
 * Single-GPU flat handles only: HNSW and vl_flat_create_multi handles return VL_ERR_INVALID_ARG.  MMR calls never join a
 * coalesced pass; the whole call holds the handle's shared lock (other searches run beside it, add / delete wait).
 * vl_last_path reports the candidate search's path. */
#define VL_MMR_MAX_FETCH 1024
int vl_index_search_mmr(const vl_index *h, uint64_t filter, const double *query, uint64_t q_len, uint64_t k,
                        uint64_t fetch_k, double lambda, int metric, uint64_t out_capacity, uint64_t *out_ids,
                        double *out_scores, uint64_t *out_n);

/* nq diversified searches against ONE index state (one hold of the reader lock): what a retrieval pipeline issues per
 * batch, fetch_k = 20 by convention.  Row i of the [nq, out_stride] outputs and out_n[i] are exactly what
 * vl_index_search_mmr(h, filter, queries + i * q_len, q_len, k, fetch_k, lambda, metric, out_capacity = out_stride, ...)
 * returns on that state: ids and f64 score bits in selection order.  out_stride acts as the single call's capacity: with
 * m = the rows the filter keeps (len without one) and n = min(fetch_k, m), a row holds min(k, n, out_stride) entries, and
 * nothing is written beyond out_n[i] entries of a row.  filter is 0, an include token or an exclusion token.
 * The argument checks are the single call's, in its order and with its texts: lambda, fetch_k < k,
 * fetch_k > VL_MMR_MAX_FETCH, the filter token, the metric, the dimension (whenever len != 0).  A NULL out_n is
 * VL_ERR_INVALID_ARG.  nq = 0 is VL_OK and writes nothing.  k = 0, out_stride = 0 or an empty (sub)index: every
 * out_n[i] = 0, VL_OK.  A failing query (VL_ERR_NAN_SCORE) makes the call return the status of the LOWEST-INDEX failing
 * query; outputs are unspecified on error.  HNSW and vl_flat_create_multi handles return VL_ERR_INVALID_ARG.  Never joins a
 * coalesced pass.
 * Route: with two or more queries, n <= 60, cosine / Euclidean / dot, a row length the batch filter has a shape for (up to
 * 768), at least 8192 rows, in-domain rows, m > 0 and no forced path, the queries of a launch sequence share ONE pass of the
 * bf16 MFMA batch filter -- over every row when filter = 0, under an exclusion token's own keep bitmap, or under a bitmap of
 * an include token's rows built on the device; no position list is read (an exclusion token's is not even built; an
 * include token's exists since its resolution) -- and each query's 64 candidates are rescored in the reference's order
 * and ranked.  The candidates scoring strictly above the exactness bound of the list's 64th key are a
 * prefix of the exact ranking; a query whose prefix holds n candidates (or whose m <= 64 rows all sit in the list) is
 * settled on the device: the pairwise similarities of those n rows and the greedy selection, in the single call's
 * arithmetic.  Otherwise (a NaN score, fewer than 64 candidates while m > 64, a query outside the fast-path domain, a zero
 * query under cosine, a shorter prefix) the single call's body answers it under the same lock, in ascending query order.
 * Everything else is a loop over the single call's body under the lock.
 * vl_last_path is VL_PATH_FAST when the pass settled any query, else the last single call's.
 * vl_index_set_mmr_batch: 0 = always the loop, 1 = the pass whenever the batch is eligible, 2 = auto (the default): the pass
 * when its estimated time is below the loop's (csrc/mmr_batch_plan.hpp; both estimates are derived).
 * vl_index_last_mmr_batch: of the last call on this handle, the queries sent to the pass, those it settled, those it handed
 * back (routed = settled + handed_back) and its launch sequences; all zero when the call looped.  Any pointer may be NULL.
 * Single-GPU flat handles only. */
int vl_index_search_mmr_batch(const vl_index *h, uint64_t filter, const double *queries, uint64_t nq, uint64_t q_len,
                              uint64_t k, uint64_t fetch_k, double lambda, int metric, uint64_t out_stride,
                              uint64_t *out_ids, double *out_scores /* [nq, out_stride] */, uint64_t *out_n /* [nq] */);
int vl_index_set_mmr_batch(vl_index *h, int mode);
int vl_index_last_mmr_batch(const vl_index *h, uint64_t *routed, uint64_t *settled, uint64_t *handed_back,
                            uint64_t *sequences);

/* NEW capability (the reference only answers in rows): the best k GROUPS, each shown by its best row -- "the best k
 * documents" over an index of chunks (group_by / collapse / search-groups elsewhere).
 * A group table maps ids to caller-chosen u64 group keys.  vl_index_groups_create: ids / group_keys [n] in any order; an id
 * repeated with the same key is fine, an id given two different keys is VL_ERR_INVALID_ARG (checked on the host before any
 * device is touched); ids the index does not hold are ignored; A ROW WHOSE ID IS NOT IN THE TABLE BELONGS TO NO GROUP AND
 * TAKES NO PART; duplicate-id rows all get their id's group.  *out_groups is a token of this handle (never 0, never
 * reused); *out_rows (may be NULL) = rows that have a group now.  Like an id filter the table is resolved on the device,
 * resolved again on the next use after add / delete, not copied by vl_index_clone and freed by vl_index_destroy.
 * vl_index_groups_rows: rows that have a group now (resolving again if rows changed) and, *out_distinct (may be NULL), the
 * distinct group keys of the table.  vl_index_groups_destroy frees the token (a search using it finishes normally).
 *
 * vl_index_search_grouped: let S be the FlatIndex holding, in storage order, the rows of h that have a group -- with
 * filter != 0 (a token of vl_index_filter_create) a row's id must be in the filter too -- and C = FlatIndex::search(query,
 * len(S), metric) on S (src/index/flat.rs:98-119; score desc, storage position asc).  Walk C from the front, emit a row
 * iff no earlier row of C has its group key, stop after k emitted rows.  Entry t = (group key, id, score) of the t-th
 * emitted row, the reference's f64 score bits.  *out_n = min(k, distinct groups in S, out_capacity); the entries are the
 * prefix of the k-answer (vl_index_search_cap's rule).  For a fixed table the answer for a smaller k is a prefix of the
 * answer for a larger one.  Only the best row of a group is returned: ask for its other rows with an id filter.
 * Errors are vl_index_search's on the WHOLE index: the dimension check runs whenever len(h) != 0, an unknown metric is
 * VL_ERR_INVALID_ARG.  VL_ERR_NAN_SCORE exactly when search(query, len(S), metric) on S would return it (a lone row never
 * compares).  k > VL_GROUPED_MAX_K, an unknown or destroyed groups token (0 included) or an unknown filter token:
 * VL_ERR_INVALID_ARG.  k = 0 or an empty S: *out_n = 0, VL_OK.
 * Single-GPU flat handles only: HNSW and vl_flat_create_multi handles return VL_ERR_INVALID_ARG.  The call never joins a
 * coalesced pass, reads the f32 slab only, and holds the handle's shared lock throughout (other searches run beside it,
 * add / delete wait).  vl_last_path: VL_PATH_FAST (two streaming passes: the best key per group, then a range search at the
 * k-th best group's score, collapsed on the device), or VL_PATH_EXACT_SORT (every score, the device-wide sort, the same
 * collapse) when k > 64, fewer than k groups have a row, a score is NaN, more rows pass the key-space threshold than the
 * candidate buffer holds (2^20), data or query lie outside the fast-path domain, or a path is forced. */
int vl_index_groups_create(vl_index *h, const uint64_t *ids, const uint64_t *group_keys, uint64_t n,
                           uint64_t *out_groups, uint64_t *out_rows);
int vl_index_groups_rows(const vl_index *h, uint64_t groups, uint64_t *out_rows, uint64_t *out_distinct);
int vl_index_groups_destroy(vl_index *h, uint64_t groups);
#define VL_GROUPED_MAX_K 1024
int vl_index_search_grouped(const vl_index *h, uint64_t groups, uint64_t filter, const double *query, uint64_t q_len,
                            uint64_t k, int metric, uint64_t out_capacity, uint64_t *out_group_keys, uint64_t *out_ids,
                            double *out_scores, uint64_t *out_n);

/* nq grouped searches against ONE index state (one hold of the reader lock): "the best k documents for each of these
 * questions" over an index of chunks.  Row i of the [nq, out_stride] outputs and out_n[i] are exactly what
 * vl_index_search_grouped(h, groups, filter, queries + i * q_len, q_len, k, metric, out_capacity = out_stride, ...) returns
 * on that state: group keys, ids and f64 score bits -- so ties come out in storage order, the answer for a smaller k is a
 * prefix of the answer for a larger one, and duplicate-id rows behave as there.  filter is 0, an include token or an
 * exclusion token, as in the single call.
 * nq = 0 is VL_OK and writes nothing.  The argument checks are the single call's, in its order and with its texts:
 * k > VL_GROUPED_MAX_K, the groups token (0 included), the filter token, the metric, the dimension (whenever len != 0);
 * then k > out_stride: VL_ERR_INVALID_ARG.  k = 0 or an empty S: every out_n[i] = 0, VL_OK.  A failing query
 * (VL_ERR_NAN_SCORE) makes the call return the status of the LOWEST-INDEX failing query; outputs are unspecified on error.
 * HNSW and vl_flat_create_multi handles return VL_ERR_INVALID_ARG.  Never joins a coalesced pass.
 * Route: with two or more queries, k <= 60, cosine / Euclidean / dot, a row length the batch filter has a shape for (up
 * to 768), at least 8192 rows, in-domain rows, a non-empty S and no forced path, the queries of a launch sequence share
 * ONE pass of the bf16 MFMA batch filter -- over every row when the table covers the index and filter = 0, else under one
 * keep bitmap of S, built on the device without a position list -- and each query's 64 candidates are rescored in the
 * reference's order, ranked, and collapsed to one row per group as far as the exactness bound certifies the ranking.  A
 * query is settled there when its certified prefix holds k groups (or S has at most 64 rows); otherwise (a NaN, a query
 * outside the fast-path domain, a zero query under cosine, too few groups in the prefix) the single call's body answers
 * it under the same lock.  Everything else is a loop over the single call's body under the lock.
 * vl_last_path is VL_PATH_FAST when the pass settled any query, else the last single call's.
 * vl_index_set_grouped_batch: 0 = always the loop, 1 = the pass whenever the batch is eligible, 2 = auto (the default):
 * the pass when its estimated time is below the loop's (csrc/grouped_batch_plan.hpp; both estimates are derived).
 * vl_index_last_grouped_batch: of the last call on this handle, the queries sent to the pass, those it settled, those it
 * handed back (routed = settled + handed_back) and its launch sequences; all zero when the call looped.  Any pointer may
 * be NULL.  Single-GPU flat handles only. */
int vl_index_search_grouped_batch(const vl_index *h, uint64_t groups, uint64_t filter, const double *queries, uint64_t nq,
                                  uint64_t q_len, uint64_t k, int metric, uint64_t out_stride, uint64_t *out_group_keys,
                                  uint64_t *out_ids, double *out_scores /* [nq, out_stride] */, uint64_t *out_n /* [nq] */);
int vl_index_set_grouped_batch(vl_index *h, int mode);
int vl_index_last_grouped_batch(const vl_index *h, uint64_t *routed, uint64_t *settled, uint64_t *handed_back,
                                uint64_t *sequences);

uint64_t vl_index_len(const vl_index *h);      /* len()       src/index/flat.rs:121-123 */
int vl_index_is_empty(const vl_index *h);      /* is_empty()  src/index/flat.rs:125-127 */
uint64_t vl_index_dimension(const vl_index *h);/* dimension() src/index/flat.rs:133-135 */

/* VectorIndexWrapper::index_type() / ::metric() (src/lib.rs:329-346): 0 = Flat, 1 = HNSW;
 * vl_index_metric returns VL_ERR_NOT_FOUND for None (flat). */
int vl_index_type(const vl_index *h);
int vl_index_metric(const vl_index *h, int *out_metric);

/* HNSW only, own extension (the reference has no ef knob): nq walks with beam width
 * max(ef, min(k, len)); outputs as vl_index_search_batch.  ef = 0 is what vl_index_search does: the reference's
 * ef = min(k, len) (src/index/hnsw.rs:437,454), raised to the handle's beam floor only if the caller set one (below).
 * The walk kernel holds beams of up to 512 entries; ef > 512 is VL_ERR_INVALID_ARG (never silently narrowed), and
 * min(k, len) > 512 is answered by the exact scan of the row store. */
int vl_index_search_ef(const vl_index *h, const double *queries, uint64_t nq, uint64_t q_len, uint64_t k,
                       uint32_t ef, int metric, uint64_t *out_ids, double *out_scores, uint64_t *out_n);

/* HNSW handle: OPT-IN beam floor of searches that name no ef.  DEFAULT 0 = the reference's rule: the walk keeps
 * ef = min(k, len) entries (src/index/hnsw.rs:437) -- 10 for k = 10.  With min_beam > 0 (at most 512) the walk keeps at
 * least that many entries and returns the best min(k, len) of them: the same number of results, recall@10 0.96
 * instead of 0.78 at N = 1 M on embedding-like data with min_beam = 32.  That is a DEVIATION from the reference's walk
 * width, which is why it is off unless asked for (env VL_HNSW_MIN_BEAM sets it for handles created afterwards). */
int vl_index_hnsw_set_min_beam(vl_index *h, uint32_t min_beam);

/* HNSW handle: how graph walks navigate.  VL_HNSW_NAV_F32 (DEFAULT) steers by f32 distances on the f32 rows and gives
 * the final beam the reference's exact u64 Metric::distance (src/index/hnsw.rs:113-174) before ordering it by
 * (u64, node).  VL_HNSW_NAV_REFERENCE (OPT-IN) makes EVERY evaluation that u64 on the f64 rows and keeps the beam in
 * (u64, first seen) order -- the searcher's insertion order for tied values -- so the walk reproduces the published
 * HNSW search as restated on the CPU (oracle/vl_hnsw_cpu.c) node for node, distance for distance, and evaluation for
 * evaluation (vl_index_hnsw_walk_stats counts exactly that walk's evaluations).  What it does NOT pin: the crate
 * `hnsw 0.11.0` itself (its source is not in the reference tree), nor the graph (built on the GPU either way).  Pinned
 * for walks of beams <= 512 only; min(k, len) > 512 is answered by the exact scan in both modes.  Each hop costs more
 * than an f32 hop (one lane walks one f64 row).  Result count, tombstones, ef and min_beam rules are
 * the same in both modes.  A clone or a reloaded index starts in VL_HNSW_NAV_F32.  VL_ERR_INVALID_ARG for a non-HNSW
 * handle or an unknown mode. */
#define VL_HNSW_NAV_F32 0
#define VL_HNSW_NAV_REFERENCE 1
int vl_index_hnsw_set_navigation(vl_index *h, int mode);

/* HNSW handle, NEW (no reference counterpart): graph walks restricted to the nodes whose id is in a set (DESIGN.md
 * section 21).  A node PASSES iff it is live and its id is in the set.  The walk navigates through every node but only
 * passing ones count: layer 0 keeps one sorted list that is cut, after every insertion, to its first `cap` entries and
 * then to the shortest prefix holding ef_walk passing entries; the answer is the passing entries of the final list, at
 * most min(k, passing nodes).  ef_walk = max(min(k, passing), ef), or the handle's beam floor when ef = 0.  Where the
 * filter is too selective for a walk (ef_walk * nodes > 256 * passing), where ef_walk > 512, or where nothing passes,
 * the answer comes from the exact scan of the passing rows instead: the true nearest passing rows in Metric::distance
 * order, post-processed like a walk's result.  With a filter every live node passes and no tombstones, a call returns
 * exactly what vl_index_search_ef returns, in either navigation mode.
 * A filter is a token of the handle that made it: never 0, never reused, not cloned, freed with the handle.  ids may be
 * unsorted and repeat; ids the index does not hold are ignored until a row with such an id is added.  Rows added or
 * deleted later are seen by the next call.  *out_nodes (may be NULL) / _filter_nodes: the nodes that pass now.
 * vl_index_filter_create still refuses HNSW handles; these tokens are no use to the flat entry points.
 * _search_ef_filtered: arguments as vl_index_search_ef plus out_stride (0 = k: entries per query the output rows hold);
 * one filter serves every query of the batch; errors are vl_index_search_ef's in the same order, then an unknown token.
 * An unknown token or a non-HNSW handle is VL_ERR_INVALID_ARG.
 * _last_filtered (any argument may be NULL): the last filtered search on the handle -- route (0 walk, 1 exact), the
 * walk's list capacity (0 on the exact route), the passing nodes, and the walks in which the capacity dropped a list
 * entry (their results may miss a passing node a wider list would have kept). */
int vl_index_hnsw_filter_create(vl_index *h, const uint64_t *ids, uint64_t n_ids, uint64_t *out_filter, uint64_t *out_nodes);
int vl_index_hnsw_filter_nodes(const vl_index *h, uint64_t filter, uint64_t *out_nodes);
int vl_index_hnsw_filter_destroy(vl_index *h, uint64_t filter);
int vl_index_search_ef_filtered(const vl_index *h, uint64_t filter, const double *queries, uint64_t nq, uint64_t q_len,
                                uint64_t k, uint32_t ef, int metric, uint64_t out_stride,
                                uint64_t *out_ids, double *out_scores, uint64_t *out_n);
int vl_index_hnsw_last_filtered(const vl_index *h, int *route, uint32_t *cap, uint64_t *pass_nodes, uint64_t *cap_cut_walks);

/* HNSW handle: the graph as it stands, every node (tombstoned ones included; node = insertion position).  level[n]
 * = top layer of each node; layer 0: cnt0[n] neighbours of node i at nbr0[i * m0 ..]; layer L >= 1 of node i: slot
 * upper_off[i] + L - 1 with cntU[slot] neighbours at nbrU[slot * m ..]; node_ids[n] the caller's ids, live[n] 0 for
 * tombstones, rows[n, dim] the f64 rows.  Any output pointer may be NULL.  The reference cannot export its graph
 * (crate hnsw 0.11.0 keeps it private; HNSWIndex::hnsw is #[serde(skip)], src/index/hnsw.rs:199-200); this is what a
 * CPU-side walk of the SAME graph needs (the repository's checker, oracle/vl_hnsw_cpu.c, is one). */
int vl_index_hnsw_graph_info(const vl_index *h, uint64_t *n_nodes, uint32_t *entry, int *max_level, uint32_t *m,
                             uint32_t *m0, uint64_t *upper_slots);
int vl_index_hnsw_graph_export(const vl_index *h, uint8_t *level, uint32_t *upper_off, uint32_t *cnt0, uint32_t *nbr0,
                               uint32_t *cntU, uint32_t *nbrU, uint64_t *node_ids, uint8_t *live, double *rows);

/* HNSW handle: the inverse of vl_index_hnsw_graph_export, on an EMPTY handle (no node yet) created with the dim, metric,
 * m, m0 and seed the graph belongs to.  Node i becomes storage position i with row rows[i * dim ..] (rows_on_device as
 * vl_index_add_bulk's values_on_device), id node_ids[i] and live[i] (0 = tombstoned, 1 = live); its lists are taken as
 * given, entry order included.  level[] and upper_off[] are NOT inputs: they follow from the level law (vl_hnsw_level)
 * and its prefix sum, n_upper must be their total, and entry / max_level are the first node of the top level.  Before
 * any device work the lists are validated on the host: counts within m0 / m, every neighbour < n, not the list's owner,
 * of a level >= the list's layer (G3), none named twice in a list (G4); a violation is VL_ERR_INVALID_ARG with the graph
 * audit's "G3: ..." / "G4: ..." text.  An id carried by two LIVE nodes is VL_ERR_DUP_ID ("Vector ID {} already exists");
 * a tombstoned node may carry any id.  What the export does not carry -- the f32 distance stored with every edge and the
 * layer-0 in-degree counter -- is recomputed on the device, bit for bit what the build stores.  *out_orphans (may be
 * NULL): nodes without an incoming layer-0 edge (reported, never refused; 0 when n < 2).  A handle that is not HNSW or
 * not empty is VL_ERR_INVALID_ARG.  Every refusal and every failure leaves the handle empty and accepting adds.  After
 * VL_OK the handle answers, exports, clones and grows like the handle the arrays were exported from. */
int vl_index_hnsw_graph_import(vl_index *h, uint64_t n, const uint64_t *node_ids, const uint8_t *live, const double *rows,
                               int rows_on_device, const uint32_t *cnt0, const uint32_t *nbr0, uint64_t n_upper,
                               const uint32_t *cntU, const uint32_t *nbrU, uint64_t *out_orphans);
/* Milliseconds of the handle's last import: out_ms[0] host validation, [1] row ingest, [2] uploads, [3] the edge-key
 * kernel, [4] the in-degree kernel (HIP events around the kernels, the host clock around the rest). */
int vl_index_hnsw_import_times(const vl_index *h, double *out_ms5);
/* HNSW handle: the four build parameters (vl_hnsw_create_ex); any pointer may be NULL. */
int vl_index_hnsw_params(const vl_index *h, uint32_t *m, uint32_t *m0, uint32_t *ef_construction, uint64_t *seed);
/* The level law: the top layer (0 .. 15) of the node at insertion position `node` in an index of that seed and m. */
int vl_hnsw_level(uint64_t seed, uint64_t node, uint32_t m);

/* get_vector(id) (src/index/flat.rs:129-131): first row with that id -> out[dim];
 * VL_ERR_NOT_FOUND stands for None. */
int vl_index_get_vector(const vl_index *h, uint64_t id, double *out_values);

/* max_id() (src/index/flat.rs:76-78): VL_ERR_NOT_FOUND stands for None (empty index). */
int vl_index_max_id(const vl_index *h, uint64_t *out_id);

/* Rows in storage order, for Serialize (src/index/flat.rs:59): ids[len], values[len, dim].
 * HNSW handle: the live rows in insertion order (the `vector_values` member, src/index/hnsw.rs:197-214). */
int vl_index_export(const vl_index *h, uint64_t *out_ids, double *out_values);

/* ---- .vlc collection files (src/persistence.rs:149-176; the step before the path) --------- */

/* load_collection_from_file without materialising CollectionData: the file is mapped, one structural
 * pass locates every row's `values` / `text` / `metadata` tokens, header.version and header.format
 * are validated after the document has been accepted (the reference's order), and the numbers are
 * converted by host threads straight into staging blocks that are ingested on the device.
 * vl_vlc_open does host work only (usable without a GPU); vl_vlc_build_index creates the GPU index
 * ("Flat" payload: FlatIndex{dim, data} taken as is, duplicate ids kept, src/index/flat.rs:59;
 * "HNSW" payload: every vector re-inserted, src/index/hnsw.rs:272-360, in file order). */
typedef struct vl_vlc_doc vl_vlc_doc;
int vl_vlc_open(const char *path, vl_vlc_doc **out);
void vl_vlc_close(vl_vlc_doc *doc);
const char *vl_vlc_name(const vl_vlc_doc *doc); /* metadata.name, UTF-8; valid until vl_vlc_close */
/* index_type 0 = Flat / 1 = HNSW; metric -1 for Flat; dim = the payload's dim; rows = vectors found;
 * vector_count / dimension = the metadata block's fields (informational, like the reference). */
int vl_vlc_info(const vl_vlc_doc *doc, int *index_type, int *metric, uint64_t *dim, uint64_t *rows,
                uint64_t *vector_count, uint64_t *dimension);
/* Per row, file order: id and the byte ranges (offset, length) in the file of its `text` string token
 * (quotes included) and `metadata` value token; length 0 = absent.  Arrays of `rows` entries. */
int vl_vlc_side_table(const vl_vlc_doc *doc, uint64_t *ids, uint64_t *text_off, uint64_t *text_len,
                      uint64_t *meta_off, uint64_t *meta_len);
/* rows [first, first + n) converted to out[n, dim] f64 on the host (correctly rounded). */
int vl_vlc_read_values(const vl_vlc_doc *doc, uint64_t first, uint64_t n, double *out_values);
int vl_vlc_build_index(const vl_vlc_doc *doc, int device, vl_index **out);

/* ---- multi-GPU row shards (no reference counterpart) ---------------------- */

/* Like vl_index_search but returns storage POSITIONS (0-based, this shard) instead of ids,
 * so that a caller holding contiguous row shards can merge per-shard top-k by
 * (score desc, shard offset + position asc) -- the reference's stable order. */
int vl_index_search_positions(const vl_index *h, const double *query, uint64_t q_len, uint64_t k, int metric,
                              uint64_t *out_pos, uint64_t *out_ids, double *out_scores, uint64_t *out_n);

/* Batched form of vl_index_search_positions: out_pos/out_ids/out_scores are [nq, k], out_n is [nq]. */
int vl_index_search_batch_positions(const vl_index *h, const double *queries, uint64_t nq, uint64_t q_len,
                                    uint64_t k, int metric, uint64_t *out_pos, uint64_t *out_ids,
                                    double *out_scores, uint64_t *out_n);

/* vl_index_search_batch_positions with the queries ALREADY IN DEVICE MEMORY of the index's GPU (e.g. embeddings computed
 * there, or a batch another rank broadcast with RCCL): d_queries is a device pointer to [nq, q_len] f64, the outputs stay
 * host buffers ([nq, k] / [nq]; out_pos and out_ids may each be NULL).  Batches the bf16 MFMA filter serves (cosine, dot,
 * Euclidean; >= 2 queries; an index of >= 8192 rows with dim <= 768) are staged by a kernel -- no host staging, no PCIe copy
 * of the queries; anything else (Manhattan, one query, a small index, an HNSW handle, queries the filter cannot certify) is
 * copied to the host and answered exactly as vl_index_search_batch would.  Same results, same errors as the host form.
 * The caller keeps d_queries valid and unmodified until the call returns (work already queued on other streams that
 * writes it must have completed). */
int vl_index_search_batch_dev(const vl_index *h, const double *d_queries, uint64_t nq, uint64_t q_len, uint64_t k,
                              int metric, uint64_t *out_pos, uint64_t *out_ids, double *out_scores, uint64_t *out_n);

/* The caller's whole step (src/client.rs:393-401: embed -> index.search) for a batch: `embeddings` is [nq, dim] f32 as the
 * model emits it (host pointer, or a device pointer on the index's GPU when embeddings_on_device != 0).  Each query is
 * widened to f64 and, with normalize != 0, L2-normalised on the device with the arithmetic of src/embeddings.rs:169-181
 * (bit for bit, like vl_index_add_embeddings_f32 does for rows), then searched through vl_index_search_batch_dev: with
 * device embeddings the batch never visits the host, with host embeddings PCIe carries 4 bytes per value instead of 8.
 * Outputs as vl_index_search_batch; row i is exactly vl_index_search of the processed query i. */
int vl_index_search_batch_embeddings_f32(const vl_index *h, const float *embeddings, uint64_t nq, uint64_t dim,
                                         int normalize, int embeddings_on_device, uint64_t k, int metric,
                                         uint64_t *out_ids, double *out_scores, uint64_t *out_n);

/* ---- row-sharded batched search over RCCL (north_star's config 3; no reference counterpart) ----------
 *
 * One process per GPU.  Rank r holds the contiguous row range [offset_r, offset_r + len_r) of the corpus as an
 * ordinary flat handle (vl_flat_create + vl_index_add_bulk ...).  A batch is answered by every rank on its own
 * shard with the single-GPU pipeline (exact f64 scores), ONE ncclAllGather over xGMI exchanges the per-shard
 * top-k records, and a device kernel merges them by (score desc, GLOBAL position asc) -- the reference's stable
 * sort (src/index/flat.rs:116) applied to the whole corpus, so the answer is bit-identical to one index holding
 * every row.  All ranks must make the same calls with the same queries / k / metric; errors of any one shard
 * travel inside the exchange, so every rank returns the same status and nobody is left waiting.  That covers the
 * local search (status in word 0 of the record) and the growth of the exchange buffers (a pre-flight status
 * all-gather through buffers made at vl_comm_create, run by every rank exactly when the buffers have to grow); a
 * device failure that leaves a rank no way to join a collective ends in ncclCommAbort on that rank -- its peers'
 * collective fails instead of waiting -- and the communicator then refuses every later call (VL_ERR_DEVICE).
 *
 * vl_comm_unique_id: rank 0 makes the ncclUniqueId and hands the 128 bytes to the other ranks by whatever
 * channel the host has (the Rust server would use its own RPC; the Python harness broadcasts it with
 * torch.distributed).  vl_comm_create is collective (ncclCommInitRank). */
#define VL_COMM_ID_BYTES 128
typedef struct vl_comm vl_comm;
int vl_comm_unique_id(uint8_t *out_id);
int vl_comm_create(const uint8_t *id, int world, int rank, int device, vl_comm **out);
void vl_comm_destroy(vl_comm *comm);
int vl_comm_world(const vl_comm *comm);
int vl_comm_rank(const vl_comm *comm);

/* Where a batch's time goes on this rank, summed over the vl_shard_search_batch* calls since the last read: the
 * local search (host clock) and, from HIP events on the exchange stream, the H2D copy of this rank's record, the
 * ncclAllGather over xGMI, and the merge kernel + D2H of the answer.  Reading clears the totals. */
int vl_comm_profile_enable(vl_comm *comm, int enable);
int vl_comm_profile_read(vl_comm *comm, uint64_t *calls, double *local_ms, double *h2d_ms, double *allgather_ms,
                         double *merge_ms);

/* How this rank's exchange records were made, since the communicator was created: on_device = batches whose record the
 * finalize kernel wrote straight into the all-gather's send buffer (only the 32-byte header then crosses PCIe in front of
 * the collective; round 4), via_host = batches that built it in pinned host memory and copied it over (Manhattan, tiny
 * shards, k > 60, failures travelling in word 0).  Either pointer may be NULL. */
int vl_comm_record_paths(const vl_comm *comm, uint64_t *on_device, uint64_t *via_host);

/* Collective: the ranks exchange (len, dimension) of their shards; each learns the global position of its
 * first row (*out_offset, rank order) and the total row count.  Call after building the shards and again
 * after any add/delete on any of them; a shard that changed since is reported as VL_ERR_INVALID_ARG by the
 * next search on every rank. */
int vl_shard_sync(const vl_index *shard, vl_comm *comm, uint64_t *out_offset, uint64_t *out_total);

/* Collective: nq searches over the WHOLE sharded corpus; outputs as vl_index_search_batch ([nq, k], row
 * stride k; out_n[q] = min(k, total rows)), identical on every rank.  out_gpos (optional) receives global
 * storage positions.  Semantics per query are FlatIndex::search's (src/index/flat.rs:98-119) on the union:
 * empty corpus accepts any q_len; otherwise q_len != dim -> VL_ERR_DIM_MISMATCH; NaN -> VL_ERR_NAN_SCORE. */
int vl_shard_search_batch(const vl_index *shard, vl_comm *comm, const double *queries, uint64_t nq, uint64_t q_len,
                          uint64_t k, int metric, uint64_t *out_gpos, uint64_t *out_ids, double *out_scores,
                          uint64_t *out_n);

/* vl_shard_search_batch with the queries already in this rank's GPU memory (e.g. one rank embedded the batch and
 * ncclBroadcast it): the local search is vl_index_search_batch_dev.  Every rank of a call uses the same form. */
int vl_shard_search_batch_dev(const vl_index *shard, vl_comm *comm, const double *d_queries, uint64_t nq, uint64_t q_len,
                              uint64_t k, int metric, uint64_t *out_gpos, uint64_t *out_ids, double *out_scores,
                              uint64_t *out_n);

/* The two halves of vl_shard_search_batch for a host that moves the records with its own transport (MPI, gloo,
 * the server's RPC): vl_shard_search_local fills this shard's exchange record (vl_shard_packed_words(nq, ks)
 * u64 words; ks = min(k, longest shard); the local status travels in word 0 and the call itself returns VL_OK
 * unless an argument is null), the host gathers the `world` records in rank order, and vl_shard_merge runs the
 * same device merge kernel on them. */
uint64_t vl_shard_packed_words(uint64_t nq, uint64_t ks);
int vl_shard_search_local(const vl_index *shard, uint64_t row_offset, int corpus_has_rows, const double *queries,
                          uint64_t nq, uint64_t q_len, uint64_t ks, int metric, uint64_t *out_packed);
/* ... the same with device-resident queries (vl_index_search_batch_dev underneath) */
int vl_shard_search_local_dev(const vl_index *shard, uint64_t row_offset, int corpus_has_rows, const double *d_queries,
                              uint64_t nq, uint64_t q_len, uint64_t ks, int metric, uint64_t *out_packed);
int vl_shard_merge(int device, const uint64_t *gathered, uint32_t world, uint64_t nq, uint64_t ks, uint64_t k,
                   uint64_t *out_gpos, uint64_t *out_ids, double *out_scores, uint64_t *out_n);

/* ---- HNSW distance callbacks (src/index/hnsw.rs:113-174) ------------------ */

/* For each of the m stored rows at `positions`, Metric::distance(query, row) -> u64
 * (trunc(dist * 1000), Rust `as u64` saturation), computed on the device in the
 * reference's f64 operation order. */
int vl_index_hnsw_distances(const vl_index *h, const double *query, uint64_t q_len, int metric,
                            const uint64_t *positions, uint64_t m, uint64_t *out_dist);

/* convert_distance_to_similarity(d_u64 as f64 / 1000.0, metric) (src/index/hnsw.rs:51-75, :478-479). */
double vl_hnsw_score(uint64_t d_u64, int metric);

/* ---- diagnostics ---------------------------------------------------------- */

const char *vl_last_error(void);                                 /* thread-local message */
void vl_last_dim_mismatch(uint64_t *expected, uint64_t *actual); /* of the last VL_ERR_DIM_MISMATCH on this thread */
int vl_last_path(void);                                          /* vl_path of the last search on this thread */

/* Force every search onto an exact pipeline (testing): 0 = automatic, 2 / 3 = vl_path value. */
int vl_index_force_path(vl_index *h, int path);

/* Single-query candidate filter: 0 = stream the f32 slab only;
 * 1 = stream a bf16 copy of the slab first (half the HBM bytes) and fall back to the f32 scan when
 * the exactness bound cannot certify the answer (switches itself off for good once more than a third of
 * 64+ tries failed);
 * 2 = auto (new handles; VL_SINGLE_FILTER=f32|bf16|auto|i8 sets the start mode): the ladder int8 -> bf16 -> f32.
 * The int8 copy first when the metric is cosine or dot and the f32 slab is at least 1 GiB
 * (VL_SINGLE_FILTER_I8_MIN_MB; VL_SINGLE_FILTER_MIN_MB does not lower it); a query it cannot certify goes on to the
 * bf16 copy when the f32 slab is at least 512 MiB (VL_SINGLE_FILTER_MIN_MB), else to the f32 slab.  Each stage is off
 * while more than a third of its last 64 tries failed to certify, re-tried every 16th search while off;
 * 3 = the int8 copy first, always (cosine and dot; mode 1's one-way switch-off), then the f32 slab.
 * The int8 copy (+0.25 x the f32 slab) and the bf16 copy (+0.5 x) are built on the first search that uses them.
 * Results are identical in every mode. */
int vl_index_set_single_filter(vl_index *h, int mode);

/* Coalescing of concurrent vl_index_search calls, flat or HNSW handle (the reference serves searches
 * concurrently under RwLock::read, src/client.rs:398; src/server.rs:269 -- one full scan each).
 * max_batch >= 2: callers that arrive while a scan is in flight are answered together by the next
 * slab pass / graph-walk launch (at most max_batch per pass; vl_index_search_batch's kernels); each caller still gets
 * exactly the result and status a lone vl_index_search returns.  window_us > 0 additionally lets a
 * lone caller wait that long for company.  max_batch 0/1 = off.
 * DEFAULT (round 4): ON with max_batch 256 and window 0 for every handle -- the reference's many-readers usage
 * (16 threads on one 10 M x 384 index: 456 QPS / 35 ms per query with separate scans, 9.8 k QPS / 1.6 ms coalesced,
 * identical answers); a lone caller finds no pass in flight, leads a pass of one and runs exactly the single-search
 * path (no wait, no batch kernels).  The first pass that answers two or more queries on an index of >= 8192 rows
 * builds the batch filter's bf16 copy of the rows (+2 bytes per value).  VL_COALESCE=0 in the
 * environment makes handles created afterwards start with it off; vl_index_set_coalescing(h, 0, 0) turns it off.
 * vl_index_coalesce_stats: passes run and queries answered by them since creation.
 * ADAPTIVE GATHER (window 0 only; on by default, VL_COALESCE_ADAPTIVE=0 or vl_index_coalesce_gather(h, 0, ..) turns it
 * off): N callers in a closed loop otherwise fall into passes of 1 and N - 1 in turn (the first caller back leads at
 * once, alone).  Every pass leaves an estimate of the callers in the loop (requests answered + compatible requests queued
 * behind it); a leader that finds fewer queued than the larger of the last two estimates waits for them, at most a quarter
 * of the recent pass time and never more than 400 us -- and only while requests arrive faster during a gather than going
 * at once would answer them (many more threads than cores: the peers sit in the run queue, the leader goes); a lone
 * caller (estimates 1, 1) never waits.  Native threads on one 10 M x 384 index: 16 -> 11.5 k QPS at 1.39 ms, 64 -> 39 k,
 * 256 -> 67 k (tools/concurrent_native.py).
 * vl_index_coalesce_gather: adaptive = 1 / 0 sets the switch, -1 leaves it; waits / waited_us (may be NULL) report the
 * passes whose leader waited and the microseconds spent waiting since creation. */
int vl_index_set_coalescing(vl_index *h, int max_batch, int window_us);
int vl_index_coalesce_stats(const vl_index *h, uint64_t *batches, uint64_t *queries);
int vl_index_coalesce_gather(vl_index *h, int adaptive, uint64_t *waits, uint64_t *waited_us);

/* HNSW handle: queries walked and Metric::distance evaluations (src/index/hnsw.rs:113-174) made for them since
 * creation: navigation evaluations on the f32 rows (dim x 4 bytes each) plus one exact f64 evaluation per entry of
 * the final beam (dim x 8 bytes each). */
int vl_index_hnsw_walk_stats(const vl_index *h, uint64_t *queries, uint64_t *distance_evals);

/* Kernel timing with HIP events on the stream the scan kernel runs on.
 * enable != 0 starts accumulating; vl_index_profile_read returns and clears the totals. */
int vl_index_profile_enable(vl_index *h, int enable);
int vl_index_profile_read(vl_index *h, uint64_t *n_scan_launches, double *scan_ms_total,
                          uint64_t *scan_bytes_total);

/* Which instantiation of the f32 scan kernel answered the last single search on this handle: variant = G * 10000 +
 * VPL * 100 + U of k_scan<metric, G, VPL, U> (negative: k_scan_generic's G), the number of workgroups it was launched
 * on, and whether the query travelled in the kernel arguments.  bench.py ties its PMC traffic figure to these. */
int vl_index_last_scan(const vl_index *h, int *variant, int *grid, int *query_in_kernarg);

/* The last launch sequence of the batch filter (bf16 MFMA, k_mfma_rows) on this handle, out6 = {K steps of 16 (row stride
 * / 16), metric, query chunks, workgroups per chunk of the last pass-1 stage, pass-1 stages, 32-row blocks sampled}; all
 * zero before the first such batch.  bench.py ties the PMC traffic figures of configs 3 and 5 to these. */
int vl_index_last_filter(const vl_index *h, int *out6);

/* Library/version probe; also reports how many HIP devices are visible (0 -> no GPU). */
int vl_runtime_info(int *n_devices, int *abi_version);

#ifdef __cplusplus
}
#endif
#endif /* VECTORLITE_AMD_H */
