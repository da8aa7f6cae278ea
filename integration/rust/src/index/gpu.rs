//! GPU-resident indexes for vectorlite: `impl VectorIndex` over libvectorlite_amd.so
//! (C ABI: include/vectorlite_amd.h of the vectorlite_amd repository).
//!
//! NOT compiled in the repository that ships it (its image has no Rust toolchain); every `extern`
//! signature below is checked against the header by tests/test_rust_binding_signatures.py.
//!
//! Vectors live in HBM (f64 master rows + an f32 scan slab); `text` / `metadata` stay on the host in a
//! side table keyed by id and are re-attached to the k winners only (the CPU FlatIndex clones them for
//! all N rows before sorting).
use std::collections::HashMap;
use std::ffi::CStr;
use std::os::raw::{c_char, c_int};

use serde::{Deserialize, Deserializer, Serialize, Serializer};

use crate::errors::{VectorLiteError, VectorLiteResult};
use crate::{SearchResult, SimilarityMetric, Vector, VectorIndex};

#[repr(C)]
pub struct vl_index {
    _private: [u8; 0],
}
#[repr(C)]
pub struct vl_vlc_doc {
    _private: [u8; 0],
}
#[repr(C)]
pub struct vl_comm {
    _private: [u8; 0],
}

extern "C" {
    fn vl_flat_create(dim: u64, device: c_int, out: *mut *mut vl_index) -> c_int;
    fn vl_flat_from_rows(dim: u64, ids: *const u64, values: *const f64, n: u64, device: c_int, out: *mut *mut vl_index) -> c_int;
    fn vl_hnsw_create(dim: u64, metric: c_int, device: c_int, out: *mut *mut vl_index) -> c_int;
    fn vl_index_clone(h: *const vl_index, out: *mut *mut vl_index) -> c_int;
    fn vl_index_destroy(h: *mut vl_index);
    fn vl_index_add(h: *mut vl_index, id: u64, values: *const f64, len: u64) -> c_int;
    fn vl_index_add_bulk(h: *mut vl_index, ids: *const u64, values: *const f64, n: u64, validate: c_int, values_on_device: c_int) -> c_int;
    fn vl_index_add_embeddings_f32(h: *mut vl_index, ids: *const u64, embeddings: *const f32, n: u64, normalize: c_int, validate: c_int, embeddings_on_device: c_int) -> c_int;
    fn vl_index_delete(h: *mut vl_index, id: u64) -> c_int;
    fn vl_index_delete_bulk(h: *mut vl_index, ids: *const u64, n_ids: u64, out_removed: *mut u64) -> c_int;
    fn vl_index_set_delete_bounce(h: *mut vl_index, bytes: u64) -> c_int;
    fn vl_index_last_delete(h: *const vl_index, out6: *mut u64) -> c_int;
    fn vl_index_update(h: *mut vl_index, id: u64, values: *const f64, len: u64) -> c_int;
    fn vl_index_update_bulk(h: *mut vl_index, ids: *const u64, values: *const f64, n: u64, insert_missing: c_int, out_updated: *mut u64, out_inserted: *mut u64) -> c_int;
    fn vl_index_last_update(h: *const vl_index, out7: *mut u64) -> c_int;
    fn vl_index_search(h: *const vl_index, query: *const f64, q_len: u64, k: u64, metric: c_int, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64) -> c_int;
    fn vl_index_search_cap(h: *const vl_index, query: *const f64, q_len: u64, k: u64, metric: c_int, out_capacity: u64, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64) -> c_int;
    fn vl_index_search_batch_cap(h: *const vl_index, queries: *const f64, nq: u64, q_len: u64, k: u64, metric: c_int, out_stride: u64, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64) -> c_int;
    fn vl_index_filter_create(h: *mut vl_index, ids: *const u64, n_ids: u64, out_filter: *mut u64, out_rows: *mut u64) -> c_int;
    fn vl_index_filter_create_excluding(h: *mut vl_index, ids: *const u64, n_ids: u64, out_filter: *mut u64, out_rows: *mut u64) -> c_int;
    fn vl_index_filter_destroy(h: *mut vl_index, filter: u64) -> c_int;
    fn vl_index_attr_rows(h: *const vl_index, attr: u64, out_rows: *mut u64) -> c_int;
    fn vl_index_attr_destroy(h: *mut vl_index, attr: u64) -> c_int;
    fn vl_index_set_where_route(h: *mut vl_index, mode: c_int) -> c_int;
    fn vl_index_last_where(h: *const vl_index, out4: *mut u64) -> c_int;
    fn vl_index_search_filtered(h: *const vl_index, filter: u64, query: *const f64, q_len: u64, k: u64, metric: c_int, out_capacity: u64, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64) -> c_int;
    fn vl_index_search_batch_filters(h: *const vl_index, filters: *const u64, n_filters: u64, queries: *const f64, nq: u64, q_len: u64, k: u64, metric: c_int, out_stride: u64, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64) -> c_int;
    fn vl_index_last_filtered_batch(h: *const vl_index, batched: *mut u64, single: *mut u64, exact: *mut u64, launches: *mut u64) -> c_int;
    fn vl_index_set_masked_batch(h: *mut vl_index, mode: c_int) -> c_int;
    fn vl_index_last_masked_batch(h: *const vl_index, routed: *mut u64, certified: *mut u64, redone: *mut u64, sequences: *mut u64, lists_built: *mut u64) -> c_int;
    fn vl_index_search_range(h: *const vl_index, filter: u64, query: *const f64, q_len: u64, min_score: f64, metric: c_int, out_ids: *mut u64, out_scores: *mut f64, out_capacity: u64, out_n: *mut u64, out_total: *mut u64) -> c_int;
    fn vl_index_search_range_batch(h: *const vl_index, filter: u64, queries: *const f64, nq: u64, q_len: u64, min_scores: *const f64, metric: c_int, out_stride: u64, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64, out_total: *mut u64) -> c_int;
    fn vl_index_last_range_batch(h: *const vl_index, mfma_queries: *mut u64, single_queries: *mut u64, exact_queries: *mut u64) -> c_int;
    fn vl_index_last_range_batch_candidates(h: *const vl_index, max_candidates: *mut u64) -> c_int;
    fn vl_index_groups_create(h: *mut vl_index, ids: *const u64, group_keys: *const u64, n: u64, out_groups: *mut u64, out_rows: *mut u64) -> c_int;
    fn vl_index_groups_rows(h: *const vl_index, groups: u64, out_rows: *mut u64, out_distinct: *mut u64) -> c_int;
    fn vl_index_groups_destroy(h: *mut vl_index, groups: u64) -> c_int;
    fn vl_index_search_grouped(h: *const vl_index, groups: u64, filter: u64, query: *const f64, q_len: u64, k: u64, metric: c_int, out_capacity: u64, out_group_keys: *mut u64, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64) -> c_int;
    fn vl_index_search_grouped_batch(h: *const vl_index, groups: u64, filter: u64, queries: *const f64, nq: u64, q_len: u64, k: u64, metric: c_int, out_stride: u64, out_group_keys: *mut u64, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64) -> c_int;
    fn vl_index_search_mmr(h: *const vl_index, filter: u64, query: *const f64, q_len: u64, k: u64, fetch_k: u64, lambda: f64, metric: c_int, out_capacity: u64, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64) -> c_int;
    fn vl_index_search_mmr_batch(h: *const vl_index, filter: u64, queries: *const f64, nq: u64, q_len: u64, k: u64, fetch_k: u64, lambda: f64, metric: c_int, out_stride: u64, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64) -> c_int;
    fn vl_index_set_mmr_batch(h: *mut vl_index, mode: c_int) -> c_int;
    fn vl_index_last_mmr_batch(h: *const vl_index, routed: *mut u64, settled: *mut u64, handed_back: *mut u64, sequences: *mut u64) -> c_int;
    fn vl_flat_create_multi(dim: u64, device_ids: *const c_int, n_dev: c_int, mode: c_int, out: *mut *mut vl_index) -> c_int;
    fn vl_index_len(h: *const vl_index) -> u64;
    fn vl_index_get_vector(h: *const vl_index, id: u64, out: *mut f64) -> c_int;
    fn vl_index_export(h: *const vl_index, out_ids: *mut u64, out_values: *mut f64) -> c_int;
    #[allow(dead_code)]
    fn vl_index_set_coalescing(h: *mut vl_index, max_batch: c_int, window_us: c_int) -> c_int;
    fn vl_index_search_batch(h: *const vl_index, queries: *const f64, nq: u64, q_len: u64, k: u64, metric: c_int, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64) -> c_int;
    fn vl_index_hnsw_set_navigation(h: *mut vl_index, mode: c_int) -> c_int;
    fn vl_index_search_ef(h: *const vl_index, queries: *const f64, nq: u64, q_len: u64, k: u64, ef: u32, metric: c_int, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64) -> c_int;
    fn vl_index_hnsw_filter_create(h: *mut vl_index, ids: *const u64, n_ids: u64, out_filter: *mut u64, out_nodes: *mut u64) -> c_int;
    #[allow(dead_code)]
    fn vl_index_hnsw_filter_nodes(h: *const vl_index, filter: u64, out_nodes: *mut u64) -> c_int;
    fn vl_index_hnsw_filter_destroy(h: *mut vl_index, filter: u64) -> c_int;
    fn vl_index_search_ef_filtered(h: *const vl_index, filter: u64, queries: *const f64, nq: u64, q_len: u64, k: u64, ef: u32, metric: c_int, out_stride: u64, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64) -> c_int;
    fn vl_vlc_open(path: *const c_char, out: *mut *mut vl_vlc_doc) -> c_int;
    fn vl_vlc_close(doc: *mut vl_vlc_doc);
    fn vl_vlc_build_index(doc: *const vl_vlc_doc, device: c_int, out: *mut *mut vl_index) -> c_int;
    fn vl_last_error() -> *const c_char;
    fn vl_last_dim_mismatch(expected: *mut u64, actual: *mut u64);
    // row-sharded batched search: one process per GPU, one RCCL all-gather per batch
    fn vl_comm_unique_id(out_id: *mut u8) -> c_int;
    fn vl_comm_create(id: *const u8, world: c_int, rank: c_int, device: c_int, out: *mut *mut vl_comm) -> c_int;
    fn vl_comm_destroy(comm: *mut vl_comm);
    fn vl_shard_sync(shard: *const vl_index, comm: *mut vl_comm, out_offset: *mut u64, out_total: *mut u64) -> c_int;
    fn vl_shard_search_batch(shard: *const vl_index, comm: *mut vl_comm, queries: *const f64, nq: u64, q_len: u64, k: u64, metric: c_int, out_gpos: *mut u64, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64) -> c_int;
    fn vl_shard_search_batch_dev(shard: *const vl_index, comm: *mut vl_comm, d_queries: *const f64, nq: u64, q_len: u64, k: u64, metric: c_int, out_gpos: *mut u64, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64) -> c_int;
    fn vl_index_search_batch_dev(h: *const vl_index, d_queries: *const f64, nq: u64, q_len: u64, k: u64, metric: c_int, out_pos: *mut u64, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64) -> c_int;
    fn vl_index_search_batch_embeddings_f32(h: *const vl_index, embeddings: *const f32, nq: u64, dim: u64, normalize: c_int, embeddings_on_device: c_int, k: u64, metric: c_int, out_ids: *mut u64, out_scores: *mut f64, out_n: *mut u64) -> c_int;
}

/// `vl_where_clause` of the header: one range clause of a predicate filter.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct vl_where_clause {
    pub attr: u64,
    pub lo: i64,
    pub hi: i64,
    pub negate: u32,
    pub reserved: u32,
}

// The attribute-column entry points that take int64 values or the clause struct: kinds the signature test's table does
// not hold, so these three were checked against the header by reading.
extern "C" {
    fn vl_index_attr_create(h: *mut vl_index, ids: *const u64, values: *const i64, n: u64, out_attr: *mut u64, out_rows: *mut u64) -> c_int;
    fn vl_index_attr_set(h: *mut vl_index, attr: u64, ids: *const u64, values: *const i64, n: u64) -> c_int;
    fn vl_index_filter_create_where(h: *mut vl_index, clauses: *const vl_where_clause, n_clauses: u64, out_filter: *mut u64, out_rows: *mut u64) -> c_int;
}

pub const VL_COMM_ID_BYTES: usize = 128;

const VL_OK: c_int = 0;
const VL_ERR_DIM_MISMATCH: c_int = 1;
const VL_ERR_DUP_ID: c_int = 2;
const VL_ERR_NOT_FOUND: c_int = 3;
const VL_ERR_METRIC_MISMATCH: c_int = 4;
const VL_ERR_NAN_SCORE: c_int = 5;
const VL_HNSW_NAV_F32: c_int = 0;
const VL_HNSW_NAV_REFERENCE: c_int = 1;

fn last_error() -> String {
    unsafe { CStr::from_ptr(vl_last_error()).to_string_lossy().into_owned() }
}

/// Declaration order of `enum SimilarityMetric` = the ABI's metric codes.
fn metric_code(m: SimilarityMetric) -> c_int {
    match m {
        SimilarityMetric::Cosine => 0,
        SimilarityMetric::Euclidean => 1,
        SimilarityMetric::Manhattan => 2,
        SimilarityMetric::DotProduct => 3,
    }
}

type Side = HashMap<u64, (String, Option<serde_json::Value>)>;

/// Shared body of the two index types: the handle dispatches like `VectorIndexWrapper`.
#[derive(Debug)]
struct Handle {
    raw: *mut vl_index,
    dim: usize,
    side: Side,
}
// The library takes its own locks: searches are re-entrant (callers hold RwLock::read together),
// add/delete take the handle exclusively.
unsafe impl Send for Handle {}
unsafe impl Sync for Handle {}

impl Drop for Handle {
    fn drop(&mut self) {
        unsafe { vl_index_destroy(self.raw) }
    }
}

impl Clone for Handle {
    fn clone(&self) -> Self {
        let mut raw = std::ptr::null_mut();
        let rc = unsafe { vl_index_clone(self.raw, &mut raw) };
        assert_eq!(rc, VL_OK, "vl_index_clone: {}", last_error());
        Handle { raw, dim: self.dim, side: self.side.clone() }
    }
}

impl Handle {
    fn add(&mut self, v: Vector) -> Result<(), String> {
        match unsafe { vl_index_add(self.raw, v.id, v.values.as_ptr(), v.values.len() as u64) } {
            VL_OK => {
                self.side.insert(v.id, (v.text, v.metadata));
                Ok(())
            }
            VL_ERR_DIM_MISMATCH => Err("Vector dimension mismatch".to_string()),
            VL_ERR_DUP_ID => Err(format!("Vector ID {} already exists", v.id)),
            _ => Err(last_error()),
        }
    }

    fn search(&self, query: &[f64], k: usize, metric: SimilarityMetric) -> VectorLiteResult<Vec<SearchResult>> {
        // vl_index_search_cap writes min(k, len at search time, cap) entries: the bound is this buffer's own size,
        // whatever the index length is by the time the search runs (in Rust `&mut self` on add already excludes a
        // concurrent grow; a C or Python caller has no such lock).
        let cap = k.min(self.len()).max(1);
        let (mut ids, mut scores, mut n) = (vec![0u64; cap], vec![0f64; cap], 0u64);
        let rc = unsafe {
            vl_index_search_cap(self.raw, query.as_ptr(), query.len() as u64, k as u64, metric_code(metric), cap as u64, ids.as_mut_ptr(), scores.as_mut_ptr(), &mut n)
        };
        match rc {
            VL_OK => Ok((0..n as usize)
                .map(|i| {
                    let (text, metadata) = self.side.get(&ids[i]).cloned().unwrap_or_default();
                    SearchResult { id: ids[i], score: scores[i], text, metadata }
                })
                .collect()),
            VL_ERR_DIM_MISMATCH => {
                let (mut e, mut a) = (0u64, 0u64);
                unsafe { vl_last_dim_mismatch(&mut e, &mut a) };
                Err(VectorLiteError::DimensionMismatch { expected: e as usize, actual: a as usize })
            }
            VL_ERR_METRIC_MISMATCH => Err(VectorLiteError::InternalError(last_error())), // caller maps to MetricMismatch
            VL_ERR_NAN_SCORE => panic!("NaN similarity score"), // what partial_cmp().unwrap() does on the CPU index
            _ => Err(VectorLiteError::InternalError(last_error())),
        }
    }

    fn len(&self) -> usize {
        unsafe { vl_index_len(self.raw) as usize }
    }

    fn get_vector(&self, id: u64) -> Option<Vector> {
        let mut values = vec![0f64; self.dim];
        if unsafe { vl_index_get_vector(self.raw, id, values.as_mut_ptr()) } != VL_OK {
            return None;
        }
        let (text, metadata) = self.side.get(&id).cloned().unwrap_or_default();
        Some(Vector { id, values, text, metadata })
    }

    /// (ids, row-major values) of every live row, insertion order: the serde payload.
    fn export(&self) -> (Vec<u64>, Vec<f64>) {
        let n = self.len();
        let (mut ids, mut values) = (vec![0u64; n], vec![0f64; n * self.dim]);
        if n > 0 {
            let rc = unsafe { vl_index_export(self.raw, ids.as_mut_ptr(), values.as_mut_ptr()) };
            assert_eq!(rc, VL_OK, "vl_index_export: {}", last_error());
        }
        (ids, values)
    }
}

// ------------------------------------------------------------------------------------------------
// Flat
// ------------------------------------------------------------------------------------------------
#[derive(Debug, Clone)]
pub struct GpuFlatIndex(Handle);

impl GpuFlatIndex {
    /// Mirrors `FlatIndex::new(dim, data)`: no validation of `data`.
    pub fn new(dim: usize, data: Vec<Vector>) -> Self {
        let ids: Vec<u64> = data.iter().map(|v| v.id).collect();
        let mut values = Vec::with_capacity(data.len() * dim);
        for v in &data {
            values.extend_from_slice(&v.values);
        }
        let mut raw = std::ptr::null_mut();
        let rc = unsafe { vl_flat_from_rows(dim as u64, ids.as_ptr(), values.as_ptr(), ids.len() as u64, 0, &mut raw) };
        assert_eq!(rc, VL_OK, "vl_flat_from_rows: {}", last_error());
        let mut side = Side::new();
        for v in data {
            side.entry(v.id).or_insert((v.text, v.metadata)); // first row of an id wins, like get_vector's find()
        }
        // tokio workers search concurrently under RwLock::read and share slab passes: the library does that by default
        // (up to 256 queries per pass, window 0, and a leader waits briefly for peers still on their way back from the
        // previous pass -- vl_index_coalesce_gather); vl_index_set_coalescing(raw, 0, 0) would turn it off
        GpuFlatIndex(Handle { raw, dim, side })
    }
}

/// How `GpuFlatIndex::new_multi` spreads one index over the GPUs of the node (include/vectorlite_amd.h).
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum MultiGpuMode {
    /// every GPU holds every row; concurrent `search` calls (tokio workers under `RwLock::read`, src/client.rs:398)
    /// are dealt to the least busy replica
    Replicas = 0,
    /// every GPU holds part of the rows; each search runs on all of them, exact per-shard top-k merged on the device
    RowShards = 1,
}

impl GpuFlatIndex {
    /// `FlatIndex::new(dim, data)` over several GPUs in THIS process (`vl_flat_create_multi`): the value behaves as any
    /// other `GpuFlatIndex` behind `VectorIndexWrapper` -- same trait, same results -- but the server's one
    /// `Arc<RwLock<Collection>>` (src/client.rs:243-247) now keeps all `devices` busy.  No rank processes, no id handshake.
    pub fn new_multi(dim: usize, data: Vec<Vector>, devices: &[i32], mode: MultiGpuMode) -> Self {
        let mut raw = std::ptr::null_mut();
        let devs: Vec<c_int> = devices.iter().map(|d| *d as c_int).collect();
        let rc = unsafe { vl_flat_create_multi(dim as u64, devs.as_ptr(), devs.len() as c_int, mode as c_int, &mut raw) };
        assert_eq!(rc, VL_OK, "vl_flat_create_multi: {}", last_error());
        let ids: Vec<u64> = data.iter().map(|v| v.id).collect();
        let mut values = Vec::with_capacity(data.len() * dim);
        for v in &data {
            values.extend_from_slice(&v.values);
        }
        if !ids.is_empty() {
            // FlatIndex::new validates nothing (src/index/flat.rs:68-73): validate = 0
            let rc = unsafe { vl_index_add_bulk(raw, ids.as_ptr(), values.as_ptr(), ids.len() as u64, 0, 0) };
            assert_eq!(rc, VL_OK, "vl_index_add_bulk: {}", last_error());
        }
        let mut side = Side::new();
        for v in data {
            side.entry(v.id).or_insert((v.text, v.metadata));
        }
        // coalescing is on by default, one queue per replica
        GpuFlatIndex(Handle { raw, dim, side })
    }
}

impl GpuFlatIndex {
    /// `for id in ids { self.delete(*id) }` in one call (`vl_index_delete_bulk`): the rows are found with one walk over the
    /// index's ids and each device array is compacted in one pass, however many ids go.  Absent and repeated ids are
    /// no-ops, as `retain` makes them (src/index/flat.rs:93-96).  Returns the rows removed.
    pub fn delete_many(&mut self, ids: &[u64]) -> Result<u64, String> {
        let mut removed = 0u64;
        match unsafe { vl_index_delete_bulk(self.0.raw, ids.as_ptr(), ids.len() as u64, &mut removed) } {
            VL_OK => {
                for id in ids {
                    self.0.side.remove(id);
                }
                Ok(removed)
            }
            _ => Err(last_error()),
        }
    }
    /// The last `delete_many`: rows removed, rows moved, launches that moved a segment in place, segments that went
    /// through the bounce buffer, bytes written to device memory, microseconds on the device (`vl_index_last_delete`).
    pub fn last_delete(&self) -> [u64; 6] {
        let mut out = [0u64; 6];
        unsafe { vl_index_last_delete(self.0.raw, out.as_mut_ptr()) };
        out
    }
    /// Bytes of the buffer deletes compact through; 0 = the default 64 MB (`vl_index_set_delete_bounce`, a diagnostic knob).
    pub fn set_delete_bounce(&mut self, bytes: u64) {
        unsafe { vl_index_set_delete_bounce(self.0.raw, bytes) };
    }
    /// Replace, in place, the values (and text / metadata) of the first row carrying `vector.id` (`vl_index_update`): the
    /// row keeps its position, every filter and group token its resolved state.  `Err("Vector ID {id} does not exist")`
    /// if no row carries the id; `Err("Vector dimension mismatch")` for a row of another length.
    pub fn update(&mut self, vector: Vector) -> Result<(), String> {
        match unsafe { vl_index_update(self.0.raw, vector.id, vector.values.as_ptr(), vector.values.len() as u64) } {
            VL_OK => {
                self.0.side.insert(vector.id, (vector.text, vector.metadata));
                Ok(())
            }
            _ => Err(last_error()),
        }
    }
    /// `for (id, row) in ids.zip(rows) { if contains(id) { update } else if insert_missing { add } else { fail } }` in one
    /// call, all or nothing (`vl_index_update_bulk`): `values` is `[ids.len(), dim]` row-major; a repeated id keeps its last
    /// values, an absent id is appended once.  Returns (rows rewritten, rows appended).
    pub fn update_many(&mut self, ids: &[u64], values: &[f64], insert_missing: bool) -> Result<(u64, u64), String> {
        if values.len() != ids.len() * self.0.dim {
            return Err("Vector dimension mismatch".to_string());
        }
        let (mut updated, mut inserted) = (0u64, 0u64);
        match unsafe {
            vl_index_update_bulk(self.0.raw, ids.as_ptr(), values.as_ptr(), ids.len() as u64, insert_missing as c_int, &mut updated, &mut inserted)
        } {
            VL_OK => Ok((updated, inserted)),
            _ => Err(last_error()),
        }
    }
    /// The last `update` / `update_many`: rows rewritten, rows appended, rows rewritten in the row-major bf16, the
    /// fragment-major bf16 and the int8 copy, staging chunks, microseconds on the device (`vl_index_last_update`).
    pub fn last_update(&self) -> [u64; 7] {
        let mut out = [0u64; 7];
        unsafe { vl_index_last_update(self.0.raw, out.as_mut_ptr()) };
        out
    }
}

impl GpuFlatIndex {
    /// The ingest step of `Collection::add_text` for a batch (`src/client.rs:313-345`): the embedding model's raw
    /// f32 outputs are widened and L2-normalised on the device exactly as `EmbeddingGenerator::generate_embedding`
    /// does on the host (`src/embeddings.rs:169-181`), then added row by row.  `texts[i]` / `metadata[i]` stay here.
    pub fn add_embeddings(&mut self, ids: &[u64], embeddings_f32: &[f32], texts: Vec<String>, metadata: Vec<Option<serde_json::Value>>) -> Result<(), String> {
        assert_eq!(embeddings_f32.len(), ids.len() * self.0.dim);
        let before = self.0.len();
        let rc = unsafe { vl_index_add_embeddings_f32(self.0.raw, ids.as_ptr(), embeddings_f32.as_ptr(), ids.len() as u64, 1, 1, 0) };
        let taken = self.0.len() - before; // rows in front of a duplicate id are kept, like sequential add() calls
        for ((id, t), m) in ids.iter().zip(texts).zip(metadata).take(taken) {
            self.0.side.insert(*id, (t, m));
        }
        if rc == VL_OK { Ok(()) } else { Err(last_error()) }
    }

    /// nq independent searches sharing slab passes (no reference counterpart); row i is exactly `search(queries[i])`.
    pub fn search_batch(&self, queries: &[f64], nq: usize, k: usize, metric: SimilarityMetric) -> VectorLiteResult<Vec<Vec<(u64, f64)>>> {
        let dim = self.0.dim;
        assert_eq!(queries.len(), nq * dim);
        let stride = k.min(self.len()).max(1); // rows of the output: the library writes min(k, len, stride) entries each
        let (mut ids, mut scores, mut n) = (vec![0u64; nq * stride], vec![0f64; nq * stride], vec![0u64; nq]);
        let rc = unsafe {
            vl_index_search_batch_cap(self.0.raw, queries.as_ptr(), nq as u64, dim as u64, k as u64, metric_code(metric), stride as u64, ids.as_mut_ptr(), scores.as_mut_ptr(), n.as_mut_ptr())
        };
        if rc != VL_OK {
            return Err(VectorLiteError::InternalError(last_error()));
        }
        Ok((0..nq).map(|q| (0..n[q] as usize).map(|i| (ids[q * stride + i], scores[q * stride + i])).collect()).collect())
    }

    /// `search` among the rows whose id is in `ids` only (no reference counterpart): exactly what `FlatIndex::search` returns
    /// on a FlatIndex holding just those rows in their storage order.  `where`-style metadata filters resolve to `ids` on
    /// the host side table first.  Single-GPU handles only (a multi-GPU handle returns an error).
    pub fn search_filtered(&self, ids: &[u64], query: &[f64], k: usize, metric: SimilarityMetric) -> VectorLiteResult<Vec<SearchResult>> {
        let (mut token, mut rows) = (0u64, 0u64);
        let rc = unsafe { vl_index_filter_create(self.0.raw, ids.as_ptr(), ids.len() as u64, &mut token, &mut rows) };
        if rc != VL_OK {
            return Err(VectorLiteError::InternalError(last_error()));
        }
        let cap = k.min(rows as usize).max(1);
        let (mut out_ids, mut scores, mut n) = (vec![0u64; cap], vec![0f64; cap], 0u64);
        let rc = unsafe {
            vl_index_search_filtered(self.0.raw, token, query.as_ptr(), query.len() as u64, k as u64, metric_code(metric), cap as u64, out_ids.as_mut_ptr(), scores.as_mut_ptr(), &mut n)
        };
        let err = if rc == VL_OK { String::new() } else { last_error() };
        unsafe { vl_index_filter_destroy(self.0.raw, token) };
        match rc {
            VL_OK => Ok((0..n as usize)
                .map(|i| {
                    let (text, metadata) = self.0.side.get(&out_ids[i]).cloned().unwrap_or_default();
                    SearchResult { id: out_ids[i], score: scores[i], text, metadata }
                })
                .collect()),
            VL_ERR_DIM_MISMATCH => {
                let (mut e, mut a) = (0u64, 0u64);
                unsafe { vl_last_dim_mismatch(&mut e, &mut a) };
                Err(VectorLiteError::DimensionMismatch { expected: e as usize, actual: a as usize })
            }
            VL_ERR_NAN_SCORE => panic!("NaN similarity score"),
            _ => Err(VectorLiteError::InternalError(err)),
        }
    }

    /// `search` among the rows whose id is NOT in `ids` (no reference counterpart): exactly what `FlatIndex::search` returns
    /// on a FlatIndex holding just the other rows in their storage order -- rows already shown, the query document itself,
    /// soft-deleted rows.  Single-GPU handles only (a multi-GPU handle returns an error).
    pub fn search_excluding(&self, ids: &[u64], query: &[f64], k: usize, metric: SimilarityMetric) -> VectorLiteResult<Vec<SearchResult>> {
        let (mut token, mut rows) = (0u64, 0u64);
        let rc = unsafe { vl_index_filter_create_excluding(self.0.raw, ids.as_ptr(), ids.len() as u64, &mut token, &mut rows) };
        if rc != VL_OK {
            return Err(VectorLiteError::InternalError(last_error()));
        }
        let cap = k.min(rows as usize).max(1);
        let (mut out_ids, mut scores, mut n) = (vec![0u64; cap], vec![0f64; cap], 0u64);
        let rc = unsafe {
            vl_index_search_filtered(self.0.raw, token, query.as_ptr(), query.len() as u64, k as u64, metric_code(metric), cap as u64, out_ids.as_mut_ptr(), scores.as_mut_ptr(), &mut n)
        };
        let err = if rc == VL_OK { String::new() } else { last_error() };
        unsafe { vl_index_filter_destroy(self.0.raw, token) };
        match rc {
            VL_OK => Ok((0..n as usize)
                .map(|i| {
                    let (text, metadata) = self.0.side.get(&out_ids[i]).cloned().unwrap_or_default();
                    SearchResult { id: out_ids[i], score: scores[i], text, metadata }
                })
                .collect()),
            VL_ERR_DIM_MISMATCH => {
                let (mut e, mut a) = (0u64, 0u64);
                unsafe { vl_last_dim_mismatch(&mut e, &mut a) };
                Err(VectorLiteError::DimensionMismatch { expected: e as usize, actual: a as usize })
            }
            VL_ERR_NAN_SCORE => panic!("NaN similarity score"),
            _ => Err(VectorLiteError::InternalError(err)),
        }
    }

    /// An attribute column id -> i64 (no reference counterpart; the reference's `Vector::metadata` is not searchable): the
    /// token `search_where` clauses refer to.  `ids` and `values` pair up in any order; an id with two different values is
    /// an error.  Rows whose id the column does not hold have no value.  Single-GPU handles only.
    pub fn attr_create(&self, ids: &[u64], values: &[i64]) -> VectorLiteResult<u64> {
        if ids.len() != values.len() {
            return Err(VectorLiteError::InternalError("attr_create: one value per id".to_string()));
        }
        let (mut token, mut rows) = (0u64, 0u64);
        match unsafe { vl_index_attr_create(self.0.raw, ids.as_ptr(), values.as_ptr(), ids.len() as u64, &mut token, &mut rows) } {
            VL_OK => Ok(token),
            _ => Err(VectorLiteError::InternalError(last_error())),
        }
    }

    /// Upserts pairs into a column: an id already held takes the new value.  Tokens made from the column are resolved again
    /// on their next use.  A refused call leaves the column as it was.
    pub fn attr_set(&self, attr: u64, ids: &[u64], values: &[i64]) -> VectorLiteResult<()> {
        if ids.len() != values.len() {
            return Err(VectorLiteError::InternalError("attr_set: one value per id".to_string()));
        }
        match unsafe { vl_index_attr_set(self.0.raw, attr, ids.as_ptr(), values.as_ptr(), ids.len() as u64) } {
            VL_OK => Ok(()),
            _ => Err(VectorLiteError::InternalError(last_error())),
        }
    }

    /// Rows that have a value in the column now.
    pub fn attr_rows(&self, attr: u64) -> VectorLiteResult<u64> {
        let mut rows = 0u64;
        match unsafe { vl_index_attr_rows(self.0.raw, attr, &mut rows) } {
            VL_OK => Ok(rows),
            _ => Err(VectorLiteError::InternalError(last_error())),
        }
    }

    /// Frees a column token; filters made from it keep working.
    pub fn attr_destroy(&self, attr: u64) {
        unsafe { vl_index_attr_destroy(self.0.raw, attr) };
    }

    /// `search` among the rows that pass 1 to 4 ANDed range clauses over attribute columns (no reference counterpart):
    /// a row qualifies iff for every clause it has a value v and `(lo <= v && v <= hi) != negate`.  The bitmap of the
    /// qualifying rows is computed on the device.  Single-GPU handles only.
    pub fn search_where(&self, clauses: &[vl_where_clause], query: &[f64], k: usize, metric: SimilarityMetric) -> VectorLiteResult<Vec<SearchResult>> {
        let (mut token, mut rows) = (0u64, 0u64);
        let rc = unsafe { vl_index_filter_create_where(self.0.raw, clauses.as_ptr(), clauses.len() as u64, &mut token, &mut rows) };
        if rc != VL_OK {
            return Err(VectorLiteError::InternalError(last_error()));
        }
        let cap = k.min(rows as usize).max(1);
        let (mut out_ids, mut scores, mut n) = (vec![0u64; cap], vec![0f64; cap], 0u64);
        let rc = unsafe {
            vl_index_search_filtered(self.0.raw, token, query.as_ptr(), query.len() as u64, k as u64, metric_code(metric), cap as u64, out_ids.as_mut_ptr(), scores.as_mut_ptr(), &mut n)
        };
        let err = if rc == VL_OK { String::new() } else { last_error() };
        unsafe { vl_index_filter_destroy(self.0.raw, token) };
        match rc {
            VL_OK => Ok((0..n as usize)
                .map(|i| {
                    let (text, metadata) = self.0.side.get(&out_ids[i]).cloned().unwrap_or_default();
                    SearchResult { id: out_ids[i], score: scores[i], text, metadata }
                })
                .collect()),
            VL_ERR_DIM_MISMATCH => {
                let (mut e, mut a) = (0u64, 0u64);
                unsafe { vl_last_dim_mismatch(&mut e, &mut a) };
                Err(VectorLiteError::DimensionMismatch { expected: e as usize, actual: a as usize })
            }
            VL_ERR_NAN_SCORE => panic!("NaN similarity score"),
            _ => Err(VectorLiteError::InternalError(err)),
        }
    }

    /// How a single search under a predicate token runs: 0 = auto (the masked ladder when its byte estimate is below the
    /// position list's), 1 = the list, 2 = the ladder wherever its conditions hold.  Answers are the same in every mode.
    pub fn set_where_route(&self, mode: i32) -> VectorLiteResult<()> {
        match unsafe { vl_index_set_where_route(self.0.raw, mode as c_int) } {
            VL_OK => Ok(()),
            _ => Err(VectorLiteError::InternalError(last_error())),
        }
    }

    /// The route of the last single predicate-filtered search (0 list, 1 masked ladder), the rows its token kept, and the
    /// predicate and column resolutions on this handle so far.
    pub fn last_where(&self) -> (u64, u64, u64, u64) {
        let mut out = [0u64; 4];
        unsafe { vl_index_last_where(self.0.raw, out.as_mut_ptr()) };
        (out[0], out[1], out[2], out[3])
    }

    /// A batch of filtered searches, one id set per query (no reference counterpart): entry `i` is exactly
    /// `search_filtered(filters[i], &queries[i], k, metric)`.  The (query, filter) pairs share scan launches -- a server's
    /// batch of requests from different users.  All queries must have one length.  Single-GPU handles only.
    pub fn search_batch_filtered(&self, filters: &[&[u64]], queries: &[Vec<f64>], k: usize, metric: SimilarityMetric) -> VectorLiteResult<Vec<Vec<SearchResult>>> {
        let nq = queries.len();
        if nq == 0 {
            return Ok(Vec::new());
        }
        let q_len = queries[0].len();
        if filters.len() != nq || queries.iter().any(|q| q.len() != q_len) {
            return Err(VectorLiteError::InternalError("search_batch_filtered: one id set per query, queries of one length".to_string()));
        }
        let mut tokens: Vec<u64> = Vec::with_capacity(nq);
        let destroy = |tokens: &[u64]| {
            for &t in tokens {
                unsafe { vl_index_filter_destroy(self.0.raw, t) };
            }
        };
        let mut most_rows = 0u64;
        for ids in filters {
            let (mut token, mut rows) = (0u64, 0u64);
            let rc = unsafe { vl_index_filter_create(self.0.raw, ids.as_ptr(), ids.len() as u64, &mut token, &mut rows) };
            if rc != VL_OK {
                let err = last_error();
                destroy(&tokens);
                return Err(VectorLiteError::InternalError(err));
            }
            tokens.push(token);
            most_rows = most_rows.max(rows);
        }
        let stride = k.min(most_rows as usize).max(1);
        let flat: Vec<f64> = queries.iter().flat_map(|q| q.iter().copied()).collect();
        let (mut out_ids, mut scores, mut n) = (vec![0u64; nq * stride], vec![0f64; nq * stride], vec![0u64; nq]);
        let rc = unsafe {
            vl_index_search_batch_filters(self.0.raw, tokens.as_ptr(), nq as u64, flat.as_ptr(), nq as u64, q_len as u64, k as u64, metric_code(metric), stride as u64, out_ids.as_mut_ptr(), scores.as_mut_ptr(), n.as_mut_ptr())
        };
        let err = if rc == VL_OK { String::new() } else { last_error() };
        destroy(&tokens);
        match rc {
            VL_OK => Ok((0..nq)
                .map(|qi| {
                    (0..n[qi] as usize)
                        .map(|i| {
                            let id = out_ids[qi * stride + i];
                            let (text, metadata) = self.0.side.get(&id).cloned().unwrap_or_default();
                            SearchResult { id, score: scores[qi * stride + i], text, metadata }
                        })
                        .collect()
                })
                .collect()),
            VL_ERR_DIM_MISMATCH => {
                let (mut e, mut a) = (0u64, 0u64);
                unsafe { vl_last_dim_mismatch(&mut e, &mut a) };
                Err(VectorLiteError::DimensionMismatch { expected: e as usize, actual: a as usize })
            }
            VL_ERR_NAN_SCORE => panic!("NaN similarity score"),
            _ => Err(VectorLiteError::InternalError(err)),
        }
    }

    /// Routing of the last filtered batch: jobs answered by a batched launch, jobs handed to the single filtered search,
    /// jobs a batched launch could not certify (redone exactly), and the batched scan launches.
    pub fn last_filtered_batch(&self) -> (u64, u64, u64, u64) {
        let (mut a, mut b, mut c, mut d) = (0u64, 0u64, 0u64, 0u64);
        unsafe { vl_index_last_filtered_batch(self.0.raw, &mut a, &mut b, &mut c, &mut d) };
        (a, b, c, d)
    }

    /// How filtered batches answer queries under exclusion tokens: 0 = with the jobs launches, 1 = every eligible query with
    /// the mask-aware MFMA batch pass, 2 = the pass when it is estimated to be faster (what new handles start in).  The
    /// answers are the same in every mode.  Single-GPU flat handles only.
    pub fn set_masked_batch(&self, mode: i32) -> VectorLiteResult<()> {
        match unsafe { vl_index_set_masked_batch(self.0.raw, mode as c_int) } {
            VL_OK => Ok(()),
            _ => Err(VectorLiteError::InternalError(last_error())),
        }
    }

    /// Of the last filtered batch: queries sent to the mask-aware MFMA pass, those it answered, those it handed back to the
    /// jobs, its launch sequences, and the position lists of exclusion tokens the call had to build.
    pub fn last_masked_batch(&self) -> (u64, u64, u64, u64, u64) {
        let (mut a, mut b, mut c, mut d, mut e) = (0u64, 0u64, 0u64, 0u64, 0u64);
        unsafe { vl_index_last_masked_batch(self.0.raw, &mut a, &mut b, &mut c, &mut d, &mut e) };
        (a, b, c, d, e)
    }

    /// `search_range` for a batch of queries against one index state (no reference counterpart): entry `i` holds at most
    /// `limit` results of `search_range(queries[i], min_scores[i], metric, ..)` and the number of rows that qualify.
    /// All queries must have the index's dimension.  Single-GPU handles only.
    pub fn search_range_batch(&self, queries: &[Vec<f64>], min_scores: &[f64], metric: SimilarityMetric, limit: usize) -> VectorLiteResult<Vec<(Vec<SearchResult>, usize)>> {
        let nq = queries.len();
        if nq == 0 {
            return Ok(Vec::new());
        }
        let q_len = queries[0].len();
        if min_scores.len() != nq || queries.iter().any(|q| q.len() != q_len) {
            return Err(VectorLiteError::InternalError("search_range_batch: one threshold per query, queries of one length".to_string()));
        }
        let flat: Vec<f64> = queries.iter().flat_map(|q| q.iter().copied()).collect();
        let (mut out_ids, mut scores) = (vec![0u64; (nq * limit).max(1)], vec![0f64; (nq * limit).max(1)]);
        let (mut n, mut total) = (vec![0u64; nq], vec![0u64; nq]);
        let rc = unsafe {
            vl_index_search_range_batch(self.0.raw, 0, flat.as_ptr(), nq as u64, q_len as u64, min_scores.as_ptr(), metric_code(metric), limit as u64, out_ids.as_mut_ptr(), scores.as_mut_ptr(), n.as_mut_ptr(), total.as_mut_ptr())
        };
        match rc {
            VL_OK => Ok((0..nq)
                .map(|qi| {
                    let results = (0..n[qi] as usize)
                        .map(|i| {
                            let id = out_ids[qi * limit + i];
                            let (text, metadata) = self.0.side.get(&id).cloned().unwrap_or_default();
                            SearchResult { id, score: scores[qi * limit + i], text, metadata }
                        })
                        .collect();
                    (results, total[qi] as usize)
                })
                .collect()),
            VL_ERR_DIM_MISMATCH => {
                let (mut e, mut a) = (0u64, 0u64);
                unsafe { vl_last_dim_mismatch(&mut e, &mut a) };
                Err(VectorLiteError::DimensionMismatch { expected: e as usize, actual: a as usize })
            }
            VL_ERR_NAN_SCORE => panic!("NaN similarity score"),
            _ => Err(VectorLiteError::InternalError(last_error())),
        }
    }

    /// Routing of the last `search_range_batch`: queries answered by the MFMA pass, the single-query fast route, the exact
    /// route, and the largest candidate count the MFMA pass kept for one query.
    pub fn last_range_batch(&self) -> (u64, u64, u64, u64) {
        let (mut a, mut b, mut c, mut d) = (0u64, 0u64, 0u64, 0u64);
        unsafe {
            vl_index_last_range_batch(self.0.raw, &mut a, &mut b, &mut c);
            vl_index_last_range_batch_candidates(self.0.raw, &mut d);
        }
        (a, b, c, d)
    }

    /// Every row whose score is at least `min_score` (no reference counterpart): the longest prefix of
    /// `FlatIndex::search(query, len, metric)` whose scores satisfy `score >= min_score`, at most `limit` of them (None: all).
    /// Returns the results and the number of rows that qualify.  Single-GPU handles only.
    pub fn search_range(&self, query: &[f64], min_score: f64, metric: SimilarityMetric, limit: Option<usize>) -> VectorLiteResult<(Vec<SearchResult>, usize)> {
        let mut cap = limit.unwrap_or(1024);
        loop {
            let (mut out_ids, mut scores, mut n, mut total) = (vec![0u64; cap.max(1)], vec![0f64; cap.max(1)], 0u64, 0u64);
            let rc = unsafe {
                vl_index_search_range(self.0.raw, 0, query.as_ptr(), query.len() as u64, min_score, metric_code(metric), out_ids.as_mut_ptr(), scores.as_mut_ptr(), cap as u64, &mut n, &mut total)
            };
            match rc {
                VL_OK => {
                    if limit.is_none() && total as usize > cap {
                        cap = total as usize; // rows arrived since the count: ask again with room for all of them
                        continue;
                    }
                    let results = (0..n as usize)
                        .map(|i| {
                            let (text, metadata) = self.0.side.get(&out_ids[i]).cloned().unwrap_or_default();
                            SearchResult { id: out_ids[i], score: scores[i], text, metadata }
                        })
                        .collect();
                    return Ok((results, total as usize));
                }
                VL_ERR_DIM_MISMATCH => {
                    let (mut e, mut a) = (0u64, 0u64);
                    unsafe { vl_last_dim_mismatch(&mut e, &mut a) };
                    return Err(VectorLiteError::DimensionMismatch { expected: e as usize, actual: a as usize });
                }
                VL_ERR_NAN_SCORE => panic!("NaN similarity score"),
                _ => return Err(VectorLiteError::InternalError(last_error())),
            }
        }
    }

    /// The best `k` groups, each shown by its best row (no reference counterpart): `pairs` maps ids to caller-chosen group
    /// keys ("chunk -> document"); rows whose id is not among them take no part.  Entry `t` is the group key and the first
    /// row of that group in `FlatIndex::search`'s order over the grouped rows.  `k <= 1024`.  Single-GPU handles only.
    /// ONE-SHOT: every call builds the table (a host sort of the pairs), resolves it on the device (a binary search per
    /// stored row, one synchronisation) and destroys it again, which at millions of pairs costs far more than the search.
    /// A caller that asks more than once keeps the token: `vl_index_groups_create` once, `vl_index_search_grouped` per
    /// query, `vl_index_groups_destroy` at the end (the table follows `add` / `delete` by itself).
    pub fn search_grouped(&self, pairs: &[(u64, u64)], query: &[f64], k: usize, metric: SimilarityMetric) -> VectorLiteResult<Vec<(u64, SearchResult)>> {
        let ids: Vec<u64> = pairs.iter().map(|p| p.0).collect();
        let keys: Vec<u64> = pairs.iter().map(|p| p.1).collect();
        let (mut token, mut rows) = (0u64, 0u64);
        let rc = unsafe { vl_index_groups_create(self.0.raw, ids.as_ptr(), keys.as_ptr(), ids.len() as u64, &mut token, &mut rows) };
        if rc != VL_OK {
            return Err(VectorLiteError::InternalError(last_error()));
        }
        let cap = k.min(rows as usize).max(1);
        let (mut out_keys, mut out_ids, mut scores, mut n) = (vec![0u64; cap], vec![0u64; cap], vec![0f64; cap], 0u64);
        let rc = unsafe {
            vl_index_search_grouped(self.0.raw, token, 0, query.as_ptr(), query.len() as u64, k as u64, metric_code(metric), cap as u64, out_keys.as_mut_ptr(), out_ids.as_mut_ptr(), scores.as_mut_ptr(), &mut n)
        };
        let err = if rc == VL_OK { String::new() } else { last_error() };
        unsafe { vl_index_groups_destroy(self.0.raw, token) };
        match rc {
            VL_OK => Ok((0..n as usize)
                .map(|i| {
                    let (text, metadata) = self.0.side.get(&out_ids[i]).cloned().unwrap_or_default();
                    (out_keys[i], SearchResult { id: out_ids[i], score: scores[i], text, metadata })
                })
                .collect()),
            VL_ERR_DIM_MISMATCH => {
                let (mut e, mut a) = (0u64, 0u64);
                unsafe { vl_last_dim_mismatch(&mut e, &mut a) };
                Err(VectorLiteError::DimensionMismatch { expected: e as usize, actual: a as usize })
            }
            VL_ERR_NAN_SCORE => panic!("NaN similarity score"),
            _ => Err(VectorLiteError::InternalError(err)),
        }
    }

    /// `search_grouped` for a batch of queries against one index state (no reference counterpart): entry `i` is
    /// `search_grouped(pairs, queries[i], k, metric)`.  The table is built once for the whole batch; eligible batches share
    /// passes of the bf16 MFMA batch filter (`vl_index_set_grouped_batch`), every other one loops under one lock.  All
    /// queries must have the index's dimension.  `k <= 1024`.  Single-GPU handles only.
    pub fn search_grouped_batch(&self, pairs: &[(u64, u64)], queries: &[Vec<f64>], k: usize, metric: SimilarityMetric) -> VectorLiteResult<Vec<Vec<(u64, SearchResult)>>> {
        let nq = queries.len();
        if nq == 0 {
            return Ok(Vec::new());
        }
        let q_len = queries[0].len();
        if queries.iter().any(|q| q.len() != q_len) {
            return Err(VectorLiteError::InternalError("search_grouped_batch: queries of one length".to_string()));
        }
        let ids: Vec<u64> = pairs.iter().map(|p| p.0).collect();
        let keys: Vec<u64> = pairs.iter().map(|p| p.1).collect();
        let (mut token, mut rows) = (0u64, 0u64);
        let rc = unsafe { vl_index_groups_create(self.0.raw, ids.as_ptr(), keys.as_ptr(), ids.len() as u64, &mut token, &mut rows) };
        if rc != VL_OK {
            return Err(VectorLiteError::InternalError(last_error()));
        }
        let flat: Vec<f64> = queries.iter().flat_map(|q| q.iter().copied()).collect();
        let stride = k.min(1024);
        let len = (nq * stride).max(1);
        let (mut out_keys, mut out_ids, mut scores, mut n) = (vec![0u64; len], vec![0u64; len], vec![0f64; len], vec![0u64; nq]);
        let rc = unsafe {
            vl_index_search_grouped_batch(self.0.raw, token, 0, flat.as_ptr(), nq as u64, q_len as u64, k as u64, metric_code(metric), stride as u64, out_keys.as_mut_ptr(), out_ids.as_mut_ptr(), scores.as_mut_ptr(), n.as_mut_ptr())
        };
        let err = if rc == VL_OK { String::new() } else { last_error() };
        unsafe { vl_index_groups_destroy(self.0.raw, token) };
        match rc {
            VL_OK => Ok((0..nq)
                .map(|qi| {
                    (0..n[qi] as usize)
                        .map(|i| {
                            let id = out_ids[qi * stride + i];
                            let (text, metadata) = self.0.side.get(&id).cloned().unwrap_or_default();
                            (out_keys[qi * stride + i], SearchResult { id, score: scores[qi * stride + i], text, metadata })
                        })
                        .collect()
                })
                .collect()),
            VL_ERR_DIM_MISMATCH => {
                let (mut e, mut a) = (0u64, 0u64);
                unsafe { vl_last_dim_mismatch(&mut e, &mut a) };
                Err(VectorLiteError::DimensionMismatch { expected: e as usize, actual: a as usize })
            }
            VL_ERR_NAN_SCORE => panic!("NaN similarity score"),
            _ => Err(VectorLiteError::InternalError(err)),
        }
    }

    /// `k` results that are relevant but not `k` copies of one paragraph (no reference counterpart): maximal marginal
    /// relevance over the exact candidates `FlatIndex::search(query, fetch_k, metric)` -- the best one first, then the
    /// candidate maximising `lambda * score - (1 - lambda) * (largest similarity to anything chosen)`.  Results come in
    /// selection order with the candidates' search scores; `lambda = 1` is the plain top `k`.  `fetch_k` in `k..=1024`.
    /// Single-GPU handles only.
    pub fn search_mmr(&self, query: &[f64], k: usize, fetch_k: usize, lambda: f64, metric: SimilarityMetric) -> VectorLiteResult<Vec<SearchResult>> {
        let cap = k.max(1);
        let (mut out_ids, mut scores, mut n) = (vec![0u64; cap], vec![0f64; cap], 0u64);
        let rc = unsafe {
            vl_index_search_mmr(self.0.raw, 0, query.as_ptr(), query.len() as u64, k as u64, fetch_k as u64, lambda, metric_code(metric), cap as u64, out_ids.as_mut_ptr(), scores.as_mut_ptr(), &mut n)
        };
        match rc {
            VL_OK => Ok((0..n as usize)
                .map(|i| {
                    let (text, metadata) = self.0.side.get(&out_ids[i]).cloned().unwrap_or_default();
                    SearchResult { id: out_ids[i], score: scores[i], text, metadata }
                })
                .collect()),
            VL_ERR_DIM_MISMATCH => {
                let (mut e, mut a) = (0u64, 0u64);
                unsafe { vl_last_dim_mismatch(&mut e, &mut a) };
                Err(VectorLiteError::DimensionMismatch { expected: e as usize, actual: a as usize })
            }
            VL_ERR_NAN_SCORE => panic!("NaN similarity score"),
            _ => Err(VectorLiteError::InternalError(last_error())),
        }
    }

    /// `search_mmr` for a batch of queries against one index state (no reference counterpart): entry `i` is
    /// `search_mmr(queries[i], k, fetch_k, lambda, metric)`.  Eligible batches share passes of the bf16 MFMA batch filter
    /// (`vl_index_set_mmr_batch`), every other one loops under one lock.  All queries must have the index's dimension.
    /// Single-GPU handles only.
    pub fn search_mmr_batch(&self, queries: &[Vec<f64>], k: usize, fetch_k: usize, lambda: f64, metric: SimilarityMetric) -> VectorLiteResult<Vec<Vec<SearchResult>>> {
        let nq = queries.len();
        if nq == 0 {
            return Ok(Vec::new());
        }
        let q_len = queries[0].len();
        if queries.iter().any(|q| q.len() != q_len) {
            return Err(VectorLiteError::InternalError("search_mmr_batch: queries of one length".to_string()));
        }
        let flat: Vec<f64> = queries.iter().flat_map(|q| q.iter().copied()).collect();
        let stride = k.min(1024);
        let len = (nq * stride).max(1);
        let (mut out_ids, mut scores, mut n) = (vec![0u64; len], vec![0f64; len], vec![0u64; nq]);
        let rc = unsafe {
            vl_index_search_mmr_batch(self.0.raw, 0, flat.as_ptr(), nq as u64, q_len as u64, k as u64, fetch_k as u64, lambda, metric_code(metric), stride as u64, out_ids.as_mut_ptr(), scores.as_mut_ptr(), n.as_mut_ptr())
        };
        match rc {
            VL_OK => Ok((0..nq)
                .map(|qi| {
                    (0..n[qi] as usize)
                        .map(|i| {
                            let id = out_ids[qi * stride + i];
                            let (text, metadata) = self.0.side.get(&id).cloned().unwrap_or_default();
                            SearchResult { id, score: scores[qi * stride + i], text, metadata }
                        })
                        .collect()
                })
                .collect()),
            VL_ERR_DIM_MISMATCH => {
                let (mut e, mut a) = (0u64, 0u64);
                unsafe { vl_last_dim_mismatch(&mut e, &mut a) };
                Err(VectorLiteError::DimensionMismatch { expected: e as usize, actual: a as usize })
            }
            VL_ERR_NAN_SCORE => panic!("NaN similarity score"),
            _ => Err(VectorLiteError::InternalError(last_error())),
        }
    }

    /// How `search_mmr_batch` answers an eligible batch: 0 = the loop, 1 = the MFMA pass, 2 = auto (the default).
    pub fn set_mmr_batch(&self, mode: i32) -> VectorLiteResult<()> {
        match unsafe { vl_index_set_mmr_batch(self.0.raw, mode as c_int) } {
            VL_OK => Ok(()),
            _ => Err(VectorLiteError::InternalError(last_error())),
        }
    }

    /// Of the last `search_mmr_batch`: (queries sent to the pass, settled there, handed back, launch sequences).
    pub fn last_mmr_batch(&self) -> (u64, u64, u64, u64) {
        let (mut r, mut s, mut hb, mut q) = (0u64, 0u64, 0u64, 0u64);
        unsafe { vl_index_last_mmr_batch(self.0.raw, &mut r, &mut s, &mut hb, &mut q) };
        (r, s, hb, q)
    }

    /// The embed -> search step of `Collection::search_text` (src/client.rs:393-401) for a batch: `embeddings` is `[nq, dim]`
    /// f32 as the model emits it; widening and L2 normalisation (src/embeddings.rs:169-181) run on the GPU, bit for bit.
    pub fn search_batch_embeddings(&self, embeddings: &[f32], nq: usize, k: usize, metric: SimilarityMetric, normalize: bool) -> VectorLiteResult<Vec<Vec<(u64, f64)>>> {
        let dim = self.0.dim;
        assert_eq!(embeddings.len(), nq * dim);
        let stride = k.min(self.len()).max(1);
        let (mut ids, mut scores, mut n) = (vec![0u64; nq * stride], vec![0f64; nq * stride], vec![0u64; nq]);
        let rc = unsafe {
            vl_index_search_batch_embeddings_f32(self.0.raw, embeddings.as_ptr(), nq as u64, dim as u64, normalize as c_int, 0, k.min(stride) as u64, metric_code(metric), ids.as_mut_ptr(), scores.as_mut_ptr(), n.as_mut_ptr())
        };
        if rc != VL_OK {
            return Err(VectorLiteError::InternalError(last_error()));
        }
        Ok((0..nq).map(|q| (0..n[q] as usize).map(|i| (ids[q * stride + i], scores[q * stride + i])).collect()).collect())
    }

    /// `search_batch` for queries that already sit in this GPU's memory (embeddings computed there): `d_queries` is a
    /// device pointer to `[nq, dim]` f64; no host staging, no PCIe copy of the queries on the MFMA batch path.
    ///
    /// # Safety
    /// `d_queries` must be a valid device allocation of `nq * dim` f64 on the index's GPU, not written until the call returns.
    pub unsafe fn search_batch_device(&self, d_queries: *const f64, nq: usize, k: usize, metric: SimilarityMetric) -> VectorLiteResult<Vec<Vec<(u64, f64)>>> {
        let stride = k.min(self.len()).max(1); // min(k, len) results at most; k is clamped to the buffers
        let (mut ids, mut scores, mut n) = (vec![0u64; nq * stride], vec![0f64; nq * stride], vec![0u64; nq]);
        let rc = vl_index_search_batch_dev(self.0.raw, d_queries, nq as u64, self.0.dim as u64, k.min(stride) as u64, metric_code(metric), std::ptr::null_mut(), ids.as_mut_ptr(), scores.as_mut_ptr(), n.as_mut_ptr());
        if rc != VL_OK {
            return Err(VectorLiteError::InternalError(last_error()));
        }
        Ok((0..nq).map(|q| (0..n[q] as usize).map(|i| (ids[q * stride + i], scores[q * stride + i])).collect()).collect())
    }
}

impl VectorIndex for GpuFlatIndex {
    fn add(&mut self, vector: Vector) -> Result<(), String> {
        self.0.add(vector)
    }
    fn delete(&mut self, id: u64) -> Result<(), String> {
        unsafe { vl_index_delete(self.0.raw, id) }; // a missing id is Ok for the flat index
        self.0.side.remove(&id);
        Ok(())
    }
    fn search(&self, query: &[f64], k: usize, metric: SimilarityMetric) -> VectorLiteResult<Vec<SearchResult>> {
        self.0.search(query, k, metric)
    }
    fn len(&self) -> usize {
        self.0.len()
    }
    fn is_empty(&self) -> bool {
        self.0.len() == 0
    }
    fn get_vector(&self, id: u64) -> Option<Vector> {
        self.0.get_vector(id)
    }
    fn dimension(&self) -> usize {
        self.0.dim
    }
}

/// Same on-disk payload as the CPU `FlatIndex` (`{dim, data: [Vector]}`): .vlc files stay interchangeable.
#[derive(Serialize, Deserialize)]
struct FlatPayload {
    dim: usize,
    data: Vec<Vector>,
}

impl Serialize for GpuFlatIndex {
    fn serialize<S: Serializer>(&self, s: S) -> Result<S::Ok, S::Error> {
        let (ids, values) = self.0.export();
        let dim = self.0.dim;
        let data = ids
            .iter()
            .enumerate()
            .map(|(i, &id)| {
                let (text, metadata) = self.0.side.get(&id).cloned().unwrap_or_default();
                Vector { id, values: values[i * dim..(i + 1) * dim].to_vec(), text, metadata }
            })
            .collect();
        FlatPayload { dim, data }.serialize(s)
    }
}

impl<'de> Deserialize<'de> for GpuFlatIndex {
    fn deserialize<D: Deserializer<'de>>(d: D) -> Result<Self, D::Error> {
        let p = FlatPayload::deserialize(d)?;
        Ok(GpuFlatIndex::new(p.dim, p.data))
    }
}

// ------------------------------------------------------------------------------------------------
// Row-sharded flat index: one process per GPU, this process holds the rows [offset, offset + len) of the corpus.
// Every rank calls the same methods with the same arguments (the library's all-gather is collective).
// ------------------------------------------------------------------------------------------------
pub struct ShardedGpuFlatIndex {
    shard: GpuFlatIndex,
    comm: *mut vl_comm,
    pub offset: u64,
    pub total: u64,
}
unsafe impl Send for ShardedGpuFlatIndex {}
unsafe impl Sync for ShardedGpuFlatIndex {}

impl ShardedGpuFlatIndex {
    /// Rank 0 creates the id and ships the 128 bytes to the other ranks over the server's own channel.
    pub fn unique_id() -> [u8; VL_COMM_ID_BYTES] {
        let mut id = [0u8; VL_COMM_ID_BYTES];
        let rc = unsafe { vl_comm_unique_id(id.as_mut_ptr()) };
        assert_eq!(rc, VL_OK, "vl_comm_unique_id: {}", last_error());
        id
    }

    /// Collective (ncclCommInitRank, then the length exchange).
    pub fn new(shard: GpuFlatIndex, id: &[u8; VL_COMM_ID_BYTES], world: usize, rank: usize, device: i32) -> Result<Self, String> {
        let mut comm = std::ptr::null_mut();
        if unsafe { vl_comm_create(id.as_ptr(), world as c_int, rank as c_int, device as c_int, &mut comm) } != VL_OK {
            return Err(last_error());
        }
        let mut s = ShardedGpuFlatIndex { shard, comm, offset: 0, total: 0 };
        s.sync()?;
        Ok(s)
    }

    /// Collective; call again after add/delete on any shard.
    pub fn sync(&mut self) -> Result<(), String> {
        match unsafe { vl_shard_sync(self.shard.0.raw, self.comm, &mut self.offset, &mut self.total) } {
            VL_OK => Ok(()),
            _ => Err(last_error()),
        }
    }

    pub fn shard_mut(&mut self) -> &mut GpuFlatIndex {
        &mut self.shard
    }

    /// `search_batch` for a batch that already sits in this rank's GPU memory (`d_queries`: device pointer to `[nq, dim]`
    /// f64 -- e.g. what an `ncclBroadcast` of the batch left there): no host staging, no PCIe copy of the queries.
    ///
    /// # Safety
    /// `d_queries` must be a valid device allocation of `nq * dim` f64 on the shard's GPU, not written until the call returns.
    pub unsafe fn search_batch_device(&self, d_queries: *const f64, nq: usize, k: usize, metric: SimilarityMetric) -> VectorLiteResult<Vec<Vec<(u64, f64)>>> {
        let dim = self.shard.0.dim;
        let stride = k.min(self.total as usize).max(1);
        let (mut ids, mut scores, mut n) = (vec![0u64; nq * stride], vec![0f64; nq * stride], vec![0u64; nq]);
        let rc = vl_shard_search_batch_dev(self.shard.0.raw, self.comm, d_queries, nq as u64, dim as u64, k.min(stride) as u64, metric_code(metric), std::ptr::null_mut(), ids.as_mut_ptr(), scores.as_mut_ptr(), n.as_mut_ptr());
        match rc {
            VL_OK => Ok((0..nq).map(|q| (0..n[q] as usize).map(|i| (ids[q * stride + i], scores[q * stride + i])).collect()).collect()),
            VL_ERR_DIM_MISMATCH => {
                let (mut e, mut a) = (0u64, 0u64);
                vl_last_dim_mismatch(&mut e, &mut a);
                Err(VectorLiteError::DimensionMismatch { expected: e as usize, actual: a as usize })
            }
            _ => Err(VectorLiteError::InternalError(last_error())),
        }
    }

    /// Collective: nq searches over the whole corpus; identical on every rank; row q is exactly what
    /// `FlatIndex::search(queries[q])` returns on one index holding every shard's rows in rank order.
    pub fn search_batch(&self, queries: &[f64], nq: usize, k: usize, metric: SimilarityMetric) -> VectorLiteResult<Vec<Vec<(u64, f64)>>> {
        let dim = self.shard.0.dim;
        assert_eq!(queries.len(), nq * dim);
        let stride = k.min(self.total as usize).max(1); // at most min(k, total) results; k is clamped to the buffers
        let (mut ids, mut scores, mut n) = (vec![0u64; nq * stride], vec![0f64; nq * stride], vec![0u64; nq]);
        let rc = unsafe {
            vl_shard_search_batch(self.shard.0.raw, self.comm, queries.as_ptr(), nq as u64, dim as u64, k.min(stride) as u64, metric_code(metric), std::ptr::null_mut(), ids.as_mut_ptr(), scores.as_mut_ptr(), n.as_mut_ptr())
        };
        match rc {
            VL_OK => Ok((0..nq).map(|q| (0..n[q] as usize).map(|i| (ids[q * stride + i], scores[q * stride + i])).collect()).collect()),
            VL_ERR_DIM_MISMATCH => {
                let (mut e, mut a) = (0u64, 0u64);
                unsafe { vl_last_dim_mismatch(&mut e, &mut a) };
                Err(VectorLiteError::DimensionMismatch { expected: e as usize, actual: a as usize })
            }
            _ => Err(VectorLiteError::InternalError(last_error())),
        }
    }
}

impl Drop for ShardedGpuFlatIndex {
    fn drop(&mut self) {
        unsafe { vl_comm_destroy(self.comm) };
    }
}

// ------------------------------------------------------------------------------------------------
// HNSW (graph built and walked on the GPU; tombstone deletes, ef = min(k, len), metric fixed at creation)
// ------------------------------------------------------------------------------------------------
#[derive(Debug, Clone)]
pub struct GpuHnswIndex {
    h: Handle,
    metric: SimilarityMetric,
}

impl GpuHnswIndex {
    pub fn new(dim: usize, metric: SimilarityMetric) -> Self {
        let mut raw = std::ptr::null_mut();
        let rc = unsafe { vl_hnsw_create(dim as u64, metric_code(metric), 0, &mut raw) };
        assert_eq!(rc, VL_OK, "vl_hnsw_create: {}", last_error());
        GpuHnswIndex { h: Handle { raw, dim, side: Side::new() }, metric }
    }
    pub fn metric(&self) -> SimilarityMetric {
        self.metric
    }
    /// `for id in ids { self.delete(*id)? }` under one lock (`vl_index_delete_bulk`): stops at the first id that does not
    /// exist with the reference's error (src/index/hnsw.rs:401-403); the ids before it stay deleted.  Ok: nodes tombstoned.
    pub fn delete_many(&mut self, ids: &[u64]) -> Result<u64, String> {
        let mut removed = 0u64;
        let rc = unsafe { vl_index_delete_bulk(self.h.raw, ids.as_ptr(), ids.len() as u64, &mut removed) };
        for id in &ids[..removed as usize] {
            self.h.side.remove(id);
        }
        match rc {
            VL_OK => Ok(removed),
            VL_ERR_NOT_FOUND => Err(format!("Vector ID {} does not exist", ids[removed as usize])),
            _ => Err(last_error()),
        }
    }
    /// Opt-in: walks navigate by the reference's own u64 distances with ties in first-seen order
    /// (`VL_HNSW_NAV_REFERENCE`); `false` returns to the default f32 navigation.  A clone starts in the default.
    pub fn set_reference_navigation(&mut self, on: bool) -> Result<(), String> {
        match unsafe { vl_index_hnsw_set_navigation(self.h.raw, if on { VL_HNSW_NAV_REFERENCE } else { VL_HNSW_NAV_F32 }) } {
            VL_OK => Ok(()),
            _ => Err(last_error()),
        }
    }
    /// Graph walk among the nodes whose id is in `ids` only (no reference counterpart): the walk navigates through every
    /// node but only live nodes with such an id count towards the beam of `max(ef, min(k, passing))` entries.  Filters that
    /// are too selective for a walk are answered by the exact scan of the passing rows (`vl_index_hnsw_last_filtered` tells the route).
    /// `ef = 0`: the beam `search` uses.  The query's metric must be the index's.
    pub fn search_filtered(&self, ids: &[u64], query: &[f64], k: usize, ef: u32, metric: SimilarityMetric) -> VectorLiteResult<Vec<SearchResult>> {
        let (mut token, mut nodes) = (0u64, 0u64);
        let rc = unsafe { vl_index_hnsw_filter_create(self.h.raw, ids.as_ptr(), ids.len() as u64, &mut token, &mut nodes) };
        if rc != VL_OK {
            return Err(VectorLiteError::InternalError(last_error()));
        }
        let cap = k.min(nodes as usize).max(1);
        let (mut out_ids, mut scores, mut n) = (vec![0u64; cap], vec![0f64; cap], 0u64);
        let rc = unsafe {
            vl_index_search_ef_filtered(self.h.raw, token, query.as_ptr(), 1, query.len() as u64, k.min(cap) as u64, ef, metric_code(metric), cap as u64, out_ids.as_mut_ptr(), scores.as_mut_ptr(), &mut n)
        };
        let err = if rc == VL_OK { String::new() } else { last_error() };
        unsafe { vl_index_hnsw_filter_destroy(self.h.raw, token) };
        match rc {
            VL_OK => Ok((0..n as usize)
                .map(|i| {
                    let (text, metadata) = self.h.side.get(&out_ids[i]).cloned().unwrap_or_default();
                    SearchResult { id: out_ids[i], score: scores[i], text, metadata }
                })
                .collect()),
            VL_ERR_DIM_MISMATCH => {
                let (mut e, mut a) = (0u64, 0u64);
                unsafe { vl_last_dim_mismatch(&mut e, &mut a) };
                Err(VectorLiteError::DimensionMismatch { expected: e as usize, actual: a as usize })
            }
            _ => Err(VectorLiteError::InternalError(err)),
        }
    }
    /// Bulk insert (one batched graph build on the device) for the custom Deserialize.
    pub fn add_all(&mut self, ids: &[u64], values: &[f64]) -> Result<(), String> {
        match unsafe { vl_index_add_bulk(self.h.raw, ids.as_ptr(), values.as_ptr(), ids.len() as u64, 1, 0) } {
            VL_OK => Ok(()),
            _ => Err(last_error()),
        }
    }
}

/// Same on-disk payload as the CPU `HNSWIndex` (`src/index/hnsw.rs:197-214`); its custom Deserialize only
/// reads `dim`, `metric`, `metadata` and `vector_values` (`:277-283`), so the two id maps are written as the
/// identity over the live rows.
#[derive(Serialize, Deserialize)]
struct HnswMeta {
    text: String,
    metadata: Option<serde_json::Value>,
}
#[derive(Serialize)]
struct HnswPayloadOut {
    dim: usize,
    metric: SimilarityMetric,
    id_to_index: HashMap<u64, usize>,
    index_to_id: HashMap<usize, u64>,
    metadata: HashMap<u64, HnswMeta>,
    vector_values: HashMap<u64, Vec<f64>>,
}
#[derive(Deserialize)]
struct HnswPayloadIn {
    dim: usize,
    metric: SimilarityMetric,
    metadata: HashMap<u64, HnswMeta>,
    vector_values: HashMap<u64, Vec<f64>>,
}

impl Serialize for GpuHnswIndex {
    fn serialize<S: Serializer>(&self, s: S) -> Result<S::Ok, S::Error> {
        let (ids, values) = self.h.export();
        let dim = self.h.dim;
        let mut out = HnswPayloadOut {
            dim,
            metric: self.metric,
            id_to_index: HashMap::new(),
            index_to_id: HashMap::new(),
            metadata: HashMap::new(),
            vector_values: HashMap::new(),
        };
        for (i, &id) in ids.iter().enumerate() {
            let (text, metadata) = self.h.side.get(&id).cloned().unwrap_or_default();
            out.id_to_index.insert(id, i);
            out.index_to_id.insert(i, id);
            out.metadata.insert(id, HnswMeta { text, metadata });
            out.vector_values.insert(id, values[i * dim..(i + 1) * dim].to_vec());
        }
        out.serialize(s)
    }
}

impl<'de> Deserialize<'de> for GpuHnswIndex {
    fn deserialize<D: Deserializer<'de>>(d: D) -> Result<Self, D::Error> {
        let p = HnswPayloadIn::deserialize(d)?;
        if p.dim == 0 {
            return Err(serde::de::Error::custom("Invalid dimension: cannot be 0"));
        }
        let mut idx = GpuHnswIndex::new(p.dim, p.metric);
        let mut ids = Vec::with_capacity(p.vector_values.len());
        let mut values = Vec::with_capacity(p.vector_values.len() * p.dim);
        for (id, v) in &p.vector_values {
            if v.len() != p.dim {
                return Err(serde::de::Error::custom(format!("Vector dimension mismatch: expected {}, got {}", p.dim, v.len())));
            }
            ids.push(*id);
            values.extend_from_slice(v);
        }
        idx.add_all(&ids, &values).map_err(serde::de::Error::custom)?;
        for (id, m) in p.metadata {
            idx.h.side.insert(id, (m.text, m.metadata));
        }
        Ok(idx)
    }
}

impl VectorIndex for GpuHnswIndex {
    fn add(&mut self, vector: Vector) -> Result<(), String> {
        self.h.add(vector)
    }
    fn delete(&mut self, id: u64) -> Result<(), String> {
        match unsafe { vl_index_delete(self.h.raw, id) } {
            VL_OK => {
                self.h.side.remove(&id);
                Ok(())
            }
            VL_ERR_NOT_FOUND => Err(format!("Vector ID {} does not exist", id)),
            _ => Err(last_error()),
        }
    }
    fn search(&self, query: &[f64], k: usize, metric: SimilarityMetric) -> VectorLiteResult<Vec<SearchResult>> {
        if metric != self.metric {
            return Err(VectorLiteError::MetricMismatch { requested: metric, index: self.metric });
        }
        self.h.search(query, k, metric)
    }
    fn len(&self) -> usize {
        self.h.len()
    }
    fn is_empty(&self) -> bool {
        self.h.len() == 0
    }
    fn get_vector(&self, id: u64) -> Option<Vector> {
        self.h.get_vector(id)
    }
    fn dimension(&self) -> usize {
        self.h.dim
    }
}
