// kernels.hpp -- launch interface of the gfx950 kernels (kernels.hip).
//
// Every kernel here serves the one hot path this repo implements: the distance
// scan + top-k of the reference's FlatIndex::search (src/index/flat.rs:98-119,
// metric math src/lib.rs:425-572) and the HNSW distance callbacks
// (src/index/hnsw.rs:113-174).  Paths are relative to /root/reference.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace vl {

enum Metric : int { COSINE = 0, EUCLIDEAN = 1, MANHATTAN = 2, DOT = 3 };

constexpr int KP = 64;            // candidate-list length (one entry per lane of a wave)
constexpr int KFAST_MAX = 60;     // largest k tried on the fast paths: the 64-entry candidate list must keep a margin
                                  // behind the k-th entry for the bound check to pass (checked per query; on 10 M random
                                  // unit rows one rank at the top is worth ~2e-4, the cosine bound ~5e-5)
constexpr uint32_t POS_SENTINEL = 0xFFFFFFFFu;

struct Cand32 {  // f32 candidate: scan key (larger = better) + storage position
    float key;
    uint32_t pos;
};
struct Cand64 {  // exact candidate: reference f64 score + storage position
    double key;
    uint32_t pos;
    uint32_t pad;
};

// Device -> host result block of one search.
struct SearchResultBlock {
    uint32_t n_out;
    uint32_t flags;  // RESULT_* bits
    uint32_t pos[KP];
    double score[KP];
    // completion stamp of a single search: written LAST (system-scope release) by the finalize kernel when the
    // caller passed a non-zero `seq`; the host waits on it instead of on the stream (flat_index.cpp, wait_result)
    uint32_t seq;
    uint32_t pad;
};
constexpr uint32_t RESULT_NEEDS_EXACT = 1u;  // bound check failed / tie at the cut: redo on the exact path
constexpr uint32_t RESULT_HAS_NAN = 2u;      // some score is NaN

// Device planes of a row shard's exchange record (shard.hpp) that the finalize kernel fills directly, so that the record of a
// batch never visits the host on its way into the all-gather: for query q (q0 + block index) the certified answer's
// (score bits, shard offset + position, id) at [q * ks + rank], and cnt[q] = entries offered -- 0 when the bound check did
// not certify the answer (the host redoes that query and patches its slice of the record).  cnt == nullptr: no record.
struct ShardRecordSink {
    unsigned long long* cnt = nullptr;         // [nq]
    unsigned long long* score_bits = nullptr;  // [nq, ks]
    unsigned long long* gpos = nullptr;        // [nq, ks]
    unsigned long long* ids = nullptr;         // [nq, ks]
    const unsigned long long* pos_to_id = nullptr;  // [n_rows] this shard's position -> id table on the device
    unsigned long long row_offset = 0;         // global position of the shard's first row
    uint32_t ks = 0;                           // record row stride
    uint32_t q0 = 0;                           // first query of this launch within the record
};

// Per-index device statistics maintained by the ingest kernel.
struct IngestStats {
    unsigned long long max_norm_bits;  // bits of the largest row L2 norm (f64, >= 0)
    unsigned int n_out_of_domain;      // rows outside the f32 fast-path domain
    unsigned int pad;
};

// Row flags produced by ingest.
constexpr uint8_t ROW_OUT_OF_DOMAIN = 1;

struct ScanPlan {
    int grid;      // workgroups launched (= partial lists written)
    int variant;   // which instantiation ran (diagnostics)
};

// f32 embeddings [n, dim] -> f64 rows [n, dim], widened and (normalize) L2-normalised with the host arithmetic of
// src/embeddings.rs:171-179 (sequential sum of squares, sqrt, one division per value; a zero row stays as it is).
hipError_t launch_embed_f32(hipStream_t s, const float* emb, uint64_t n, uint32_t dim, bool normalize, double* out);

// f64 master rows [n, dim] -> f32 slab rows [n, ld] (zero padded), inv_norm[n], flags[n], stats.
hipError_t launch_ingest(hipStream_t s, const double* master, float* slab, float* inv_norm, uint8_t* flags,
                         IngestStats* stats, uint64_t n, uint32_t dim, uint32_t ld);

// In-place update: staged f64 rows [m, dim] replace the master rows at the DISTINCT positions pos[0..m) (device memory), and
// their slab rows, inv_norm and flags are derived as launch_ingest derives them; out_flags[i] = the new flag of pos[i];
// stats->max_norm_bits is raised.  16-byte copies of the master row when dim is even and both arrays are 16-byte aligned.
hipError_t launch_update_rows(hipStream_t s, const double* staged, const uint32_t* pos, uint32_t m, double* master, float* slab,
                              float* inv_norm, uint8_t* flags, uint8_t* out_flags, IngestStats* stats, uint32_t dim, uint32_t ld);

// Bulk delete (delete_plan.hpp): copies `rows` rows of `pitch` bytes to dst + r * pitch, r = 0 .. rows - 1, destination
// row dst_begin + r reading source row d + #{i : keys[i] <= d} of src_base (d = dst_begin + r; keys[i] = r_i - i over the
// ascending removed positions, on the device).  [c_lo, c_hi] = the shifts of the segment's first and last row.  dst is the
// destination's place in the same array (a direct segment: the plan keeps the launch's destinations below its sources) or
// the bounce buffer.  16 bytes per lane where pitch and both addresses allow, else 8, 4 or 1.
hipError_t launch_move_rows(hipStream_t s, const void* src_base, void* dst, uint64_t pitch, const uint32_t* keys, uint32_t c_lo,
                            uint32_t c_hi, uint64_t dst_begin, uint64_t rows);

// Upper bound on the workgroups launch_scan uses (partials must hold SCAN_MAX_GRID*KP entries).
constexpr int SCAN_MAX_GRID = 4096;
constexpr int SELECT_MAX_GRID = 1024;
constexpr int SCAN_BATCH_QB = 8;           // queries served by one slab pass of k_scan_batch
constexpr int SCAN_BATCH_MAX_GRID = 2048;
constexpr int SCAN_BATCH_MAX_QUERIES = 512;  // queries one launch_scan_batch call answers: groups of QB as blockIdx.y
// partial-list buffers: the scan lists (single: SCAN_MAX_GRID; batch: QB x SCAN_BATCH_MAX_GRID),
// followed by two ping-pong merge regions of QB x 64 lists
constexpr size_t PARTIALS32_LISTS = (size_t)SCAN_BATCH_QB * SCAN_BATCH_MAX_GRID;
static_assert(PARTIALS32_LISTS >= (size_t)SCAN_MAX_GRID, "single-query lists must fit");
constexpr size_t PARTIALS32_ENTRIES = (PARTIALS32_LISTS + 2 * (size_t)SCAN_BATCH_QB * 64) * KP;
constexpr size_t PARTIALS64_ENTRIES = (size_t)(SELECT_MAX_GRID + 128) * KP;

// K1: f32 slab scan -> per-workgroup top-KP partial lists.
// Two ways to hand over the query.  q32_host != nullptr (and scan_takes_qarg(ld)): the f32 query, zero padded to
// `ld` floats, rounded from the f64 query to nearest even, is copied into the kernel arguments -- nothing has to
// be on the device before the launch.  Otherwise q64 is the f64 query in device memory and each lane rounds its
// slice itself.  Both forms produce the same keys.
constexpr int SCAN_QARG_FLOATS = 768;
bool scan_takes_qarg(uint32_t ld);
hipError_t launch_scan(hipStream_t s, int metric, const float* slab, const float* inv_norm, const double* q64,
                       uint64_t n, uint32_t dim, uint32_t ld, Cand32* partials, ScanPlan* plan,
                       const float* q32_host = nullptr);

// `out` may be pinned host memory (the result block is written once, by one wave).
// K2: merge partial lists -> top-KP, rescore them in reference f64 arithmetic from the master
// rows, rank by (score desc, pos asc), run the exactness bound check, write the result block.
// One workgroup per query: `partials` holds nq x n_lists lists (query-major), q64 is [nq, dim],
// q_norms[nq] the f64 query norms, out[nq] the result blocks.
// 60 < k <= KMULTI_MAX: the scan's workgroup lists cut into n_parts partitions of 64 candidates each, rescored and
// ranked together; out = n_parts result blocks (ranks 64 i .. 64 i + 63 in block i; n_out and flags in block 0).
constexpr int KMULTI_MAX = 220;
hipError_t launch_merge_finalize_multi(hipStream_t s, int metric, Cand32* partials, int n_lists_total, int n_parts,
                                       const double* master, const double* q64, const double* q_norm, uint32_t dim,
                                       uint64_t n_rows, uint32_t k, double max_row_norm, SearchResultBlock* out);
// q64 / q_norms may be device memory or device-visible pinned host memory (a single search reads its 3 KB query
// straight from the pinned staging block: one workgroup, one PCIe round trip hidden behind the list merge).
// seq != 0 (nq == 1 only): out->seq = seq is stored last, system-scope release, after the result block.
hipError_t launch_merge_finalize(hipStream_t s, int metric, Cand32* partials, int n_lists, int nq,
                                 const double* master, const double* q64, const double* q_norms, uint32_t dim,
                                 uint64_t n_rows, uint32_t k, double max_row_norm, SearchResultBlock* out,
                                 double in_extra = 0.0, uint32_t seq = 0, const ShardRecordSink* sink = nullptr);
// The stamped single search (nq = 1, out->seq = seq stored last) of a candidate filter whose rows carry extra input
// rounding: the filter's `in_extra` term of the bound comes last.
inline hipError_t launch_merge_finalize(hipStream_t s, uint32_t seq, int metric, Cand32* partials, int n_lists,
                                        const double* master, const double* q64, const double* q_norm, uint32_t dim,
                                        uint64_t n_rows, uint32_t k, double max_row_norm, SearchResultBlock* out,
                                        double in_extra)
{
    return launch_merge_finalize(s, metric, partials, n_lists, 1, master, q64, q_norm, dim, n_rows, k, max_row_norm, out,
                                 in_extra, seq);
}

// K2 for a batch whose candidates already are ONE sorted top-64 list per query (lists[nq][KP], the MFMA filter's output):
// the rescoring of each query's 64 rows split over four 256-thread workgroups + one wave per query that ranks, checks the
// bound and emits -- the same arithmetic and result blocks as launch_merge_finalize(n_lists = 1), at batch throughput.
// score_scratch: nq x KP doubles of device memory.
hipError_t launch_batch_finalize(hipStream_t s, int metric, const Cand32* lists, int nq, const double* master, const double* q64,
                                 const double* q_norms, uint32_t dim, uint64_t n_rows, uint32_t k, double max_row_norm,
                                 SearchResultBlock* out, double in_extra, double* score_scratch,
                                 const ShardRecordSink* sink = nullptr);

// launch_batch_finalize for lists of kept rows only (the masked MFMA filter): n_rows and k of query q
// are m_of[q] (its filter's rows, > 0) and k_of[q] = min(k, m_of[q]), two device arrays of nq words -- what
// launch_merge_finalize_jobs reads from its job table.  Any nq >= 1; no shard record.
hipError_t launch_batch_finalize_rows(hipStream_t s, int metric, const Cand32* lists, int nq, const double* master,
                                      const double* q64, const double* q_norms, uint32_t dim, const uint32_t* m_of,
                                      const uint32_t* k_of, double max_row_norm, SearchResultBlock* out, double in_extra,
                                      double* score_scratch);

// K3: one launch for nq <= SCAN_BATCH_MAX_QUERIES queries (q64 is [nq, dim]) in groups of SCAN_BATCH_QB -- every group is one
// pass over the slab (blockIdx.y = group); lists are written query-major, plan->grid of them per query (<= 64 when there is
// more than one group, so that the finalize kernel takes them without a merge level).
bool scan_batch_supported(uint32_t ld);
hipError_t launch_scan_batch(hipStream_t s, int metric, const float* slab, const float* inv_norm, const double* q64,
                             uint32_t nq, uint64_t n, uint32_t dim, uint32_t ld, Cand32* partials, ScanPlan* plan);

// Exact path: reference-order f64 score of every row.
hipError_t launch_exact_scan(hipStream_t s, int metric, const double* master, const double* q64, uint64_t n,
                             uint32_t dim, double* scores, uint32_t* nan_flag);
// Search restricted to an id filter: the rows are plist[0..m), ascending storage positions.
// K1 over the subset: the same partial lists as launch_scan (positions are storage positions, the keys k_scan's), on a grid
// sized from m.  q32_host != nullptr and scan_subset_takes_qarg(ld): the query in the kernel arguments, else q64 on the device.
// plan->variant = SUBSET_VARIANT_BASE + G * 10000 + VPL * 100 + U, or -(SUBSET_VARIANT_BASE + G) for the generic kernel.
constexpr int SUBSET_VARIANT_BASE = 3000000;
bool scan_subset_takes_qarg(uint32_t ld);
hipError_t launch_scan_subset(hipStream_t s, int metric, const float* slab, const float* inv_norm, const uint32_t* plist,
                              uint64_t m, const double* q64, uint32_t dim, uint32_t ld, Cand32* partials, ScanPlan* plan,
                              const float* q32_host = nullptr);
// Many (query, subset) jobs in one launch (batches).  A job is one row of a device table; its f64
// query is row `job` of q64 [n_jobs, dim].  The grid is (gx, n_jobs): every job writes gx lists (job-major) with
// k_scan_subset's keys and positions.  gx and the launch's membership are subset_batch_plan.hpp's; gx * n_jobs <=
// PARTIALS32_LISTS, n_jobs <= SCAN_BATCH_MAX_QUERIES, every m > 0.  No allocation, no synchronisation.
// plan->variant = SUBSET_JOBS_VARIANT_BASE + G * 10000 + VPL * 100 + U, or -(SUBSET_JOBS_VARIANT_BASE + G) for the generic kernel.
struct SubsetJobDev {
    const uint32_t* plist;  // ascending storage positions of the job's filter
    uint32_t m;             // their number, > 0
    uint32_t k;             // min(k, m)
};
constexpr int SUBSET_JOBS_VARIANT_BASE = 6000000;
hipError_t launch_scan_subset_jobs(hipStream_t s, int metric, const float* slab, const float* inv_norm, const SubsetJobDev* jobs,
                                   uint32_t n_jobs, uint32_t gx, const double* q64, uint32_t dim, uint32_t ld, Cand32* partials,
                                   ScanPlan* plan);
// launch_merge_finalize for those lists: n_rows and k of each query are its job's m and k.  More than SCAN_BATCH_QB jobs:
// n_lists <= 64 (the merge scratch behind the lists holds SCAN_BATCH_QB queries).
hipError_t launch_merge_finalize_jobs(hipStream_t s, int metric, Cand32* partials, int n_lists, const SubsetJobDev* jobs,
                                      uint32_t n_jobs, const double* master, const double* q64, const double* q_norms,
                                      uint32_t dim, double max_row_norm, SearchResultBlock* out);
// What the plan needs to know about the scan: lanes per row and row groups in flight of the stride's shape (the default
// one, or the generic kernel's), and the workgroups of that kernel resident at once (what launch_scan_subset's grid is
// capped at).
hipError_t scan_subset_jobs_shape(int metric, uint32_t ld, int* g, int* u, int* resident);
// Exact path over the subset: scores[i] = reference f64 score of row plist[i].
hipError_t launch_exact_scan_subset(hipStream_t s, int metric, const double* master, const double* q64, const uint32_t* plist,
                                    uint64_t m, uint32_t dim, double* scores, uint32_t* nan_flag);
// Resolution of an id filter against the position -> id table pos_ids[0..n): fids[0..nf) sorted, unique.  Step 1 counts the
// matches per chunk of positions and turns the counts into offsets, *m_out = total (counts: FILTER_COUNTS_MAX words); step 2
// writes the m matching positions in ascending order into plist[0..m).
constexpr int FILTER_COUNTS_MAX = 1024;
// invert (an exclusion filter): a position matches iff its id is NOT in the set; nf may then be 0.
hipError_t launch_filter_count(hipStream_t s, const unsigned long long* pos_ids, uint64_t n, const unsigned long long* fids,
                               uint64_t nf, uint32_t* counts, uint32_t* m_out, bool invert = false);
hipError_t launch_filter_compact(hipStream_t s, const unsigned long long* pos_ids, uint64_t n, const unsigned long long* fids,
                                 uint64_t nf, const uint32_t* offsets, uint64_t m, uint32_t* plist, bool invert = false);
// An exclusion filter's keep bitmap: keep[0..(n + 63) / 64), bit p & 63 of word p >> 6 set iff p < n
// and pos_ids[p] is not in the set (nf may be 0: every row kept).  include: the bit is set iff pos_ids[p] IS in the set (the
// rows of an include token as a bitmap).
hipError_t launch_filter_bits(hipStream_t s, const unsigned long long* pos_ids, uint64_t n, const unsigned long long* fids,
                              uint64_t nf, unsigned long long* keep, bool include = false);
// the exclusive scan of launch_filter_count alone: counts[0..nb) in place, nb <= FILTER_COUNTS_MAX, total -> *m_out
hipError_t launch_filter_scan(hipStream_t s, uint32_t* counts, uint32_t nb, uint32_t* m_out);

// Attribute columns and predicate filter tokens (where.hip).
// A column's resolution against pos_ids[0..n): fids[0..nf) sorted, unique, fvals[i] the value of fids[i] (nf may be 0).
// value_of_row[p] = the value of row p's id, 0 where the column does not hold it; has[0..(n + 63) / 64) in the keep bitmap's
// layout, bit set iff the column holds the row's id; *rows_out = the number of such rows.
hipError_t launch_attr_rows(hipStream_t s, const unsigned long long* pos_ids, uint64_t n, const unsigned long long* fids,
                            const long long* fvals, uint64_t nf, long long* value_of_row, unsigned long long* has, uint32_t* rows_out);
// 1 to 4 clauses, ANDed: row p qualifies iff for every clause it has a value v and (lo <= v && v <= hi) != negate.
struct WhereClausesDev {
    const long long* value_of_row[4];
    const unsigned long long* has[4];
    long long lo[4], hi[4];
    uint32_t negate[4];
    uint32_t n_clauses;
};
// One pass over the clauses' columns: keep[0..(n + 63) / 64) (bits at or past n are 0; value_of_row is not read there),
// counts[0..where_grid_for(n)) = exclusive offsets of the kept rows per chunk (where_plan.hpp: chunks of whole words),
// *m_out = kept rows.  counts holds FILTER_COUNTS_MAX words.
hipError_t launch_where_bits(hipStream_t s, uint64_t n, const WhereClausesDev& clauses, unsigned long long* keep, uint32_t* counts,
                             uint32_t* m_out);
// plist[0..m) = the positions whose keep bit is set, ascending; offsets = launch_where_bits' counts.
hipError_t launch_where_compact(hipStream_t s, uint64_t n, const unsigned long long* keep, const uint32_t* offsets, uint64_t m,
                                uint32_t* plist);

// K1 under a keep bitmap: launch_scan's partial lists without the rows whose bit is 0, on launch_scan's grid (sized from n).
// Only at the strides VL_SCAN_VARIANTS specialises (scan_masked_supported(ld)), the stride's default shape; the query as
// launch_scan_subset takes it (q32_host where scan_takes_qarg(ld), else q64 in device memory).
// plan->variant = MASK_VARIANT_BASE + G * 10000 + VPL * 100 + U.
constexpr int MASK_VARIANT_BASE = 7000000;
bool scan_masked_supported(uint32_t ld);
hipError_t launch_scan_masked(hipStream_t s, int metric, const float* slab, const float* inv_norm, const unsigned long long* keep,
                              uint64_t n, const double* q64, uint32_t dim, uint32_t ld, Cand32* partials, ScanPlan* plan,
                              const float* q32_host = nullptr);

// Range search (score >= min_score).  ctr: RANGE_CTR_WORDS words of device memory, zeroed by the
// caller in front of each sequence: [APPENDED] rows the scan appended (it keeps counting past the buffer), [TOTAL] rows
// that pass the cut, [NAN] set when a rescored row is NaN.
constexpr int RANGE_VARIANT_BASE = 4000000;
constexpr uint32_t RANGE_CAND_MAX = 1u << 20;  // C: positions the candidate buffer holds (4 MB; with scores, keys and payloads 28 MB)
constexpr uint32_t RANGE_SMALL = 2048;         // survivors ranked before the host knows their number (one workgroup's LDS sort)
constexpr int RANGE_CTR_APPENDED = 0, RANGE_CTR_TOTAL = 1, RANGE_CTR_NAN = 2, RANGE_CTR_GROUP_NAN = 3, RANGE_CTR_WORDS = 4;
// The scan that appends: cand[] receives the storage position of every row whose key is NOT <= tau (tau NaN: every row), up to
// cap of them.  plist != nullptr: over the rows plist[0..n) (an id filter's list).  Keys, query forms and grid are k_scan's.
// plan->variant = RANGE_VARIANT_BASE + G * 10000 + VPL * 100 + U, or -(RANGE_VARIANT_BASE + G) for the generic kernel.
bool scan_range_takes_qarg(uint32_t ld);
hipError_t launch_scan_range(hipStream_t s, int metric, const float* slab, const float* inv_norm, const uint32_t* plist,
                             uint64_t n, const double* q64, uint32_t dim, uint32_t ld, float tau, uint32_t* cand,
                             uint32_t cap, uint32_t* ctr, ScanPlan* plan, const float* q32_host = nullptr);
// scores[i] = reference f64 score of row cand[i], i < ctr[APPENDED]; nothing when the counter ran past cap.  q64 on the device.
hipError_t launch_range_rescore(hipStream_t s, int metric, const double* master, const double* q64, const uint32_t* cand,
                                uint32_t cap, uint32_t dim, double* scores, uint32_t* ctr);
// The cut: slots i < m with scores[i] >= min_score are appended to (keys, pv) = (descending-order key of the score,
// position << 32 | i), position = cand ? cand[i] : i; ctr[TOTAL] counts them, entries past store_cap are only counted.
// m = *m_ptr when given (nothing is done when it exceeds m_max), else m_max.
// group_of_row != nullptr (a grouped search): rows whose group_of_row[position] is GROUP_NONE are
// dropped as well; with keep_nan, NaN scores of grouped rows stay in and ctr[GROUP_NAN] counts them.
hipError_t launch_range_cut(hipStream_t s, const double* scores, const uint32_t* cand, const uint32_t* m_ptr, uint64_t m_max,
                            double min_score, uint64_t* keys, uint64_t* pv, uint64_t store_cap, uint32_t* ctr,
                            const uint32_t* group_of_row = nullptr, uint64_t n_rows = 0, bool keep_nan = false);
// Rank (keys, pv) by (score desc, position asc) and write the first min(total, k) (position, score).  total_ptr != nullptr:
// the count is still the device's -- ranks up to RANGE_SMALL survivors (more: the output is unspecified, call again with
// the count); else `total` entries, buffers of sort_capacity_for(total).
hipError_t launch_range_rank(hipStream_t s, uint64_t* keys, uint64_t* pv, const double* scores, const uint32_t* total_ptr,
                             uint64_t total, uint64_t k, uint32_t* out_pos, double* out_scores);

// Grouped search (best row per group).
// The group table's resolution beside the filter's: group_of_row[p] = dense[i] when pos_ids[p] == fids[i], else GROUP_NONE.
hipError_t launch_group_rows(hipStream_t s, const unsigned long long* pos_ids, uint64_t n, const unsigned long long* fids,
                             const uint32_t* dense, uint64_t nf, uint32_t* group_of_row);
// Pass 1: every scanned row with a group raises best[group] (zeroed by the caller) to
// ordered(key) << 32 | (0xFFFFFFFF - position).  plist != nullptr: over the rows plist[0..n).  Keys, query forms, shapes
// and grid are the range scan's.  plan->variant = GROUP_VARIANT_BASE + G * 10000 + VPL * 100 + U, or
// -(GROUP_VARIANT_BASE + G) for the generic kernel.
constexpr int GROUP_VARIANT_BASE = 5000000;
constexpr uint32_t GROUPED_MAX_K = 1024;  // VL_GROUPED_MAX_K
hipError_t launch_scan_group_best(hipStream_t s, int metric, const float* slab, const float* inv_norm, const uint32_t* plist,
                                  uint64_t n, const double* q64, uint32_t dim, uint32_t ld, const uint32_t* group_of_row,
                                  uint64_t* best, ScanPlan* plan, const float* q32_host = nullptr);
// The 64 largest values of best[0..n_groups), decoded: cand[0..c) = their positions, best first, c = min(k, non-empty
// groups, 64) -> ctr[RANGE_CTR_APPENDED] (what launch_range_rescore reads).  lists: GROUP_TOP_LISTS * KP entries of scratch.
constexpr int GROUP_TOP_LISTS = 64;
hipError_t launch_group_top(hipStream_t s, const uint64_t* best, uint64_t n_groups, uint32_t k, Cand32* lists, uint32_t* cand,
                            uint32_t* ctr);
// The collapse of n ranked survivors pv[i] = position << 32 | slot (n = *n_ptr when given -- nothing is done when it exceeds
// n_max -- else n_max): survivor i is kept iff no earlier one has its group; the first k kept are written as (group key,
// position, scores[slot]) and *out_n = their number.  first: n_groups words of scratch.
hipError_t launch_group_collapse(hipStream_t s, const uint64_t* pv, const double* scores, const uint32_t* n_ptr, uint64_t n_max,
                                 const uint32_t* group_of_row, uint64_t n_rows, const uint64_t* group_keys, uint64_t n_groups,
                                 uint32_t* first, uint32_t k, uint64_t* out_keys, uint32_t* out_pos, double* out_scores,
                                 uint32_t* out_n);

// Batched grouped search.  Device -> host block of one query of a launch sequence: entry t < n_out is
// the t-th group of the answer as (dense group number, storage position, reference score).  flags == 0: the query is
// settled and the block is its answer; RESULT_NEEDS_EXACT: the host hands the query to the single call.
struct GroupedResultBlock {
    uint32_t n_out;
    uint32_t flags;  // RESULT_* bits
    uint32_t pos[KP];
    uint32_t group[KP];
    double score[KP];
};
// launch_batch_finalize with a rank-and-collapse stage in k_batch_rank_emit's place: lists hold rows of S only (every row
// that has a group, or the rows under the sequence's one keep bitmap), n_rows = |S| > 0, 1 <= k <= KFAST_MAX.  A candidate
// is certified iff its score is > bound_for_key(the list's 64th key) -- or the list holds all n_rows <= 64 rows; the
// certified ones are collapsed to the first row of each group and the first k of those emitted.  Settled iff k groups came
// out, or the whole of S was ranked without a NaN.  group_of_row: index_rows words.
hipError_t launch_batch_finalize_grouped(hipStream_t s, int metric, const Cand32* lists, int nq, const double* master,
                                         const double* q64, const double* q_norms, uint32_t dim, uint64_t n_rows, uint32_t k,
                                         double max_row_norm, const uint32_t* group_of_row, uint64_t index_rows,
                                         GroupedResultBlock* out, double in_extra, double* score_scratch);
// The stage behind the rescoring alone, on scores the caller supplies (tests/native/grouped_batch_audit.hip).
hipError_t launch_batch_rank_collapse(hipStream_t s, int metric, const Cand32* lists, const double* scores, int nq,
                                      const double* q_norms, uint32_t ld, uint64_t n_rows, uint32_t k, double max_row_norm,
                                      const uint32_t* group_of_row, uint64_t index_rows, GroupedResultBlock* out,
                                      double in_extra);
// The keep bitmap of S (grouped.hip): bit p & 63 of keep[p >> 6] is set iff p < n, group_of_row[p] != GROUP_NONE and the
// filter keeps row p -- filter_keep (an exclusion token's own bitmap) when given, else pos_ids[p] in fids[0..nf) when
// fids != nullptr (an include token's sorted ids; nf may be 0), else every row.  *m_out (zeroed here) receives the
// number of bits set.  keep: (n + 63) / 64 words.
hipError_t launch_group_keep_bits(hipStream_t s, const uint32_t* group_of_row, uint64_t n, const unsigned long long* filter_keep,
                                  const unsigned long long* pos_ids, const unsigned long long* fids, uint64_t nf,
                                  unsigned long long* keep, uint32_t* m_out);

// k_batch_rescore alone: scores[q * KP + i] = the reference f64 score of query q against the row of lists[q * KP + i] (the
// batched MMR search runs its own stage behind it, mmr.hip).  The MFMA filter's metrics.
hipError_t launch_batch_rescore(hipStream_t s, int metric, const Cand32* lists, int nq, const double* master, const double* q64,
                                uint32_t dim, double* scores);

// Batched range search: the device tail behind launch_mfma_range_candidates.  cand / cnt / cap are
// the MFMA filter's per-query candidate buffers; ctr holds RBATCH_CTR_WORDS words per query, zeroed by the caller:
// [TOTAL] rows of the query with score >= min_scores[q], [NAN] set when a rescored row is NaN, [WANT] entries emitted for
// the query (0 when the host has to redo it: cnt[q] > cap, a NaN, or more than RBATCH_SEG survivors), [OFF] where they
// start in the packed outputs.  sv_score / sv_pos: nq x RBATCH_SEG entries of scratch.  out_pos / out_scores receive, per
// answered query, its first min(total, emit_cap) entries in (score desc, position asc) order; emit_cap <= RBATCH_SEG, so
// nq x emit_cap entries always hold them.
constexpr uint32_t RBATCH_SEG = 2048;  // survivors per query the segmented rank holds (one workgroup's LDS sort)
constexpr int RBATCH_CTR_TOTAL = 0, RBATCH_CTR_NAN = 1, RBATCH_CTR_OFF = 2, RBATCH_CTR_WANT = 3, RBATCH_CTR_WORDS = 4;
hipError_t launch_range_batch_tail(hipStream_t s, int metric, const Cand32* cand, const uint32_t* cnt, uint32_t cap, uint32_t nq,
                                   const double* master, const double* q64, const double* min_scores, uint32_t dim,
                                   uint64_t n_rows, uint32_t emit_cap, double* sv_score, uint32_t* sv_pos, uint32_t* ctr,
                                   uint32_t* out_pos, double* out_scores);

// Exact path, k <= KP: top-k of scores[] by (score desc, pos asc).
int select_grid_for(uint64_t n);
// Ranks 64 r .. 64 r + k - 1 of the exact order: `after` = the (full, k = 64) block of round r - 1, nullptr for r = 0.
hipError_t launch_exact_select(hipStream_t s, const double* scores, uint64_t n, uint32_t k, Cand64* partials,
                               const uint32_t* nan_flag, SearchResultBlock* out,
                               const SearchResultBlock* after = nullptr);
constexpr int SELECT_MAX_ROUNDS = 16;  // k <= 1024 is answered by rounds of 64; larger k by the full sort
// Exact path, any k: device-wide sort of (score desc, pos asc); writes the first k.
// okeys/opos are scratch of next_pow2(n) entries.
uint64_t sort_capacity_for(uint64_t n);
hipError_t launch_exact_sort(hipStream_t s, const double* scores, uint64_t n, uint64_t k, uint64_t* okeys,
                             uint32_t* opos, uint32_t* out_pos, double* out_scores);

// Diversified (MMR) search, DESIGN.md section 16 (mmr.hip).  Where a search left its finalised candidates in device memory:
// result blocks (entry i = blocks[i / KP].pos / .score[i % KP]: the certified finalize, the multi-list finalize, the exact
// selection rounds) or the exact sort's (pos, scores) arrays.  The kernels take the candidates only when the device says
// the search stands: blocks[0].n_out == n_block0 with neither NEEDS_EXACT nor HAS_NAN, and *nan_flag == 0 when given.
constexpr uint32_t MMR_MAX_FETCH = 1024;  // VL_MMR_MAX_FETCH: one workgroup holds rel, red and the flags in LDS
struct MmrSource {
    const SearchResultBlock* blocks = nullptr;
    const uint32_t* pos = nullptr;       // blocks == nullptr: [n]
    const double* scores = nullptr;      // blocks == nullptr: [n]
    const uint32_t* plist = nullptr;     // given: entries are indices into this id filter's position list
    const uint32_t* nan_flag = nullptr;  // the exact scan's NaN flag
    uint32_t plist_len = 0;
    uint32_t n = 0;         // candidates: min(fetch_k, rows)
    uint32_t n_block0 = 0;  // what blocks[0].n_out says when the search stands
    uint32_t n_rows = 0;    // rows of the index (positions are clamped below it)
};
// k_mmr_pairwise (sim[i][j] = calculate(metric, row[i], row[j]), i != j < n, row stride MMR_MAX_FETCH) then k_mmr_select:
// the greedy selection of min(k, n) candidates, written in selection order as (storage position, score bits) into
// out[t / KP] entry t % KP; out[0].n_out = the count, out[0].flags = NEEDS_EXACT when the candidates were not taken;
// seq != 0: out[0].seq = seq stored last, system-scope release (`out` pinned).  sim: MMR_MAX_FETCH^2 doubles.
hipError_t launch_mmr(hipStream_t s, int metric, const double* master, uint32_t dim, const MmrSource& src, double* sim,
                      uint32_t k, double lambda, SearchResultBlock* out, uint32_t seq);

// The batched form, behind k_batch_rescore: lists / scores as launch_batch_rank_collapse takes them
// (rows of S only, n_rows = |S| > 0).  k_mmr_batch_rank certifies the prefix of each query's ranking that scores strictly
// above bound_for_key(the list's 64th key) -- every candidate when the list holds all n_rows <= 64 rows -- and a query is
// settled iff no score is NaN and the prefix holds n_need = min(fetch_k, n_rows) <= KFAST_MAX candidates; its first n_need
// ranked candidates go to ranked[q] (device memory, nq blocks).  k_mmr_batch_select computes their pairwise similarities
// in LDS and selects min(k, n_need) of them as k_mmr_select does: out[q] = the chosen (storage position, score bits) in
// selection order, n_out, flags = 0; an unsettled query leaves n_out = 0 and RESULT_NEEDS_EXACT.  master: index_rows rows.
hipError_t launch_mmr_batch(hipStream_t s, int metric, const Cand32* lists, const double* scores, int nq, const double* q_norms,
                            const double* master, uint32_t dim, uint64_t n_rows, uint64_t index_rows, uint32_t n_need, uint32_t k,
                            double lambda, double max_row_norm, double in_extra, SearchResultBlock* ranked, SearchResultBlock* out);

// HNSW distance callbacks: u64 distance of query vs the rows at positions[0..m).
hipError_t launch_hnsw_distances(hipStream_t s, int metric, const double* master, const double* q64,
                                 uint32_t dim, const uint32_t* positions, uint32_t m, uint64_t* out);

}  // namespace vl
