// flat_index.hpp -- C++ host side of the GPU flat index: the mirror of the reference's
// `impl VectorIndex for FlatIndex` (src/index/flat.rs:60-135) above the HIP kernels.
// The reference is compiled code (Rust, not buildable in this image), so the host layer is
// C++; include/vectorlite_amd.h exposes it as the C ABI a Rust `impl VectorIndex` would bind.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "rwlock.hpp"
#include "attr_plan.hpp"
#include "coalescer.hpp"
#include "group_plan.hpp"
#include "kernels.hpp"
#include "mfma_scan.hpp"
#include "single_filter.hpp"

namespace vl {

// vl_status values (include/vectorlite_amd.h)
enum Status : int {
    OK = 0,
    ERR_DIM_MISMATCH = 1,
    ERR_DUP_ID = 2,
    ERR_NOT_FOUND = 3,
    ERR_METRIC_MISMATCH = 4,
    ERR_NAN_SCORE = 5,
    ERR_DEVICE = 6,
    ERR_OOM = 7,
    ERR_INVALID_ARG = 8,
};

constexpr int K3_PIPE_QUERIES = SCAN_BATCH_MAX_QUERIES;  // queries staged, launched (one scan + one finalize) and synchronised together on the f32 batch path
constexpr int COALESCE_DEFAULT_BATCH = 256;  // concurrent callers one pass answers at most, by default (window 0)

enum Path : int { PATH_NONE = 0, PATH_FAST = 1, PATH_EXACT_SELECT = 2, PATH_EXACT_SORT = 3 };

// thread-local diagnostics (vl_last_error & friends)
void set_last_error(const std::string& msg);
const char* last_error();
void set_dim_mismatch(uint64_t expected, uint64_t actual);
void get_dim_mismatch(uint64_t* expected, uint64_t* actual);
void set_last_path(int p);
int last_path();

// Per-search scratch: one HIP stream plus device/pinned buffers.  Searches are re-entrant
// (the reference searches under RwLock::read, src/client.rs:398): each call borrows one.
struct Workspace {
    int device = 0;
    hipStream_t stream = nullptr;
    double* d_q64 = nullptr;
    double* h_q64 = nullptr;  // pinned
    size_t q_cap = 0;
    Cand32* d_partials = nullptr;
    Cand64* d_partials64 = nullptr;
    SearchResultBlock* d_result = nullptr;
    SearchResultBlock* h_result = nullptr;  // pinned
    uint32_t* d_nan = nullptr;
    uint32_t* h_nan = nullptr;  // pinned
    // exact path (lazy)
    double* d_scores = nullptr;
    size_t scores_cap = 0;
    uint64_t* d_okeys = nullptr;
    uint32_t* d_opos = nullptr;
    size_t sort_cap = 0;
    uint32_t* d_out_pos = nullptr;
    double* d_out_scores = nullptr;
    size_t out_cap = 0;
    // hnsw distances (lazy)
    uint32_t* d_positions = nullptr;
    uint64_t* d_dists = nullptr;
    size_t hn_cap = 0;
    // range search (lazy): counters, the scan's candidate positions and their scores, the cut's sort keys and payloads
    uint32_t* rg_ctr = nullptr;
    uint32_t* rg_h_ctr = nullptr;    // pinned
    uint32_t* rg_cand = nullptr;     // [RANGE_CAND_MAX]
    double* rg_scores = nullptr;     // [RANGE_CAND_MAX]
    uint64_t* rg_keys = nullptr;     // [rg_sort_cap]
    uint64_t* rg_pv = nullptr;       // [rg_sort_cap]
    size_t rg_sort_cap = 0;
    uint32_t* rg_h_pos = nullptr;    // pinned [RANGE_SMALL]
    double* rg_h_scores = nullptr;   // pinned [RANGE_SMALL]
    // batched range search (lazy): per-query counters, thresholds and survivor segments of one launch sequence
    uint32_t* rb_ctr = nullptr;      // [MFMA_MAX_BATCH, RBATCH_CTR_WORDS]
    double* rb_min = nullptr;        // [MFMA_MAX_BATCH] min_scores
    double* rb_sv_score = nullptr;   // [rb_sv_queries, RBATCH_SEG]
    uint32_t* rb_sv_pos = nullptr;   // [rb_sv_queries, RBATCH_SEG]
    size_t rb_sv_queries = 0;
    float* rb_h_thr = nullptr;       // pinned [MFMA_MAX_BATCH]
    double* rb_h_min = nullptr;      // pinned [MFMA_MAX_BATCH]
    uint32_t* rb_h_ctr = nullptr;    // pinned [MFMA_MAX_BATCH, RBATCH_CTR_WORDS]
    uint32_t* rb_h_cnt = nullptr;    // pinned [MFMA_MAX_BATCH]
    uint32_t* rb_h_pos = nullptr;    // pinned [RBATCH_SPEC]: packed answers copied back before the host knows their number
    double* rb_h_scores = nullptr;   // pinned [RBATCH_SPEC]
    // grouped search (lazy): pass 1's per-group slots and the collapse's first-appearance table ([gp_cap] each), the top
    // groups' positions and reference scores, its counters, the emitted group keys
    uint64_t* gp_best = nullptr;
    uint32_t* gp_first = nullptr;
    size_t gp_cap = 0;
    Cand32* gp_lists = nullptr;      // [GROUP_TOP_LISTS, KP]
    uint32_t* gp_cand = nullptr;     // [KP]
    double* gp_scores = nullptr;     // [KP]
    uint32_t* gp_ctr = nullptr;      // [RANGE_CTR_WORDS] pass 1's, then [1] the collapse's count
    uint64_t* gp_out_keys = nullptr; // [GROUPED_MAX_K]
    uint32_t* gp_h_ctr = nullptr;    // pinned [RANGE_CTR_WORDS + 1]
    double* gp_h_scores = nullptr;   // pinned [KP]
    uint64_t* gp_h_keys = nullptr;   // pinned [GROUPED_MAX_K]
    // batched grouped search (lazy): the result blocks of two launch sequences in flight, the keep bitmap of S when a filter
    // is involved (the table's own bitmap is cached on the table), the device's count of its bits
    GroupedResultBlock* gb_h_result = nullptr;  // pinned [2][MFMA_MAX_BATCH]
    unsigned long long* gb_keep = nullptr;      // [gb_keep_cap] words
    size_t gb_keep_cap = 0;
    uint32_t* gb_m = nullptr;                   // [1]
    // diversified search (lazy): the candidates' pairwise similarities, [MMR_MAX_FETCH][MMR_MAX_FETCH] (8 MB)
    double* mmr_sim = nullptr;
    // batched diversified search (lazy): the ranked candidates of a launch sequence's queries, between its two kernels
    SearchResultBlock* mb_ranked = nullptr;  // [MFMA_MAX_BATCH]
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<float> q32;   // the f32 query handed to k_scan in its kernel arguments
    uint32_t seq = 0;         // stamp of the last single search issued from this workspace (h_result->seq)
    // f32 batch path (K3), several passes in flight: staging for K3_PIPE_QUERIES queries and their result blocks (lazy)
    double* k3_d_q64 = nullptr;                // [K3_PIPE_QUERIES, dim] queries, then their norms, then (a filtered batch) the
                                               // launch's SubsetJobDev table: k3_stage_words(dim) words
    double* k3_h_q64 = nullptr;                // pinned
    SearchResultBlock* k3_h_result = nullptr;  // pinned [K3_PIPE_QUERIES]
    // large-batch MFMA path (lazy)
    MfmaScratch mf;
    double* mf_d_q64 = nullptr;             // [MFMA_MAX_BATCH, dim] queries, then their norms
    double* mf_h_q64 = nullptr;             // pinned
    Cand32* mf_lists = nullptr;             // [MFMA_MAX_BATCH, KP]
    double* mf_scores = nullptr;            // [MFMA_MAX_BATCH, KP] reference scores of the candidates (batch finalize scratch)
    SearchResultBlock* mf_h_result = nullptr;  // pinned [2][MFMA_MAX_BATCH]: two launch sequences in flight
    unsigned char* mf_h_dom = nullptr;      // pinned [2][MFMA_MAX_BATCH]: in-domain flags of device-resident queries
    hipEvent_t mf_ev_done[2] = {nullptr, nullptr};  // behind each sequence's finalize
    hipEvent_t mf_ev_h2d = nullptr;         // behind the copies out of the pinned query staging area
    bool mf_h2d_pending = false;

    ~Workspace();
};

// words of the K3 staging buffers: per query its values and its norm, and the 16 bytes of a filtered batch's job table entry
inline size_t k3_stage_words(uint64_t dim) { return (size_t)K3_PIPE_QUERIES * (dim + 3); }

// Search scratch (streams, partial-list buffers, the batch filter's buffers: ~10 MB, 80+ MB once a large batch ran) is
// shared by every handle of one (device, dimension): the reference keeps a HashMap of collections (src/client.rs:243-247),
// and thousands of small handles each holding their own scratch held 14.6 MB apiece (tools/many_handles_probe.py).
// Reference-counted: the pool of a (device, dimension) goes when its last handle does.
struct WorkspacePool {
    std::mutex mu;
    std::vector<Workspace*> free_;
    std::vector<std::unique_ptr<Workspace>> all;
    size_t users = 0;
};

// An attribute column of one single-GPU flat handle (vl_index_attr_create): the caller's (id, int64)
// pairs as an AttrPlan, and -- resolved like a group table, stale when the handle's mutation count or the column's version
// moved -- value_of_row[position] and the "has a value" bitmap.  vl_index_attr_set swaps the plan and bumps the version
// under the index's exclusive lock, so neither moves while a search holds the shared lock.
struct AttrColumn {
    std::mutex mu;                         // guards everything below (taken after the index lock and after a filter's mutex)
    int device = 0;
    AttrPlan plan;
    uint64_t version = 1;                  // bumped by every successful vl_index_attr_set
    unsigned long long* d_ids = nullptr;   // [pairs_cap] the plan on the device
    long long* d_values = nullptr;
    uint64_t pairs_cap = 0;
    long long* d_value_of_row = nullptr;   // [rows_cap] 0 where the row has no value
    uint64_t rows_cap = 0;
    unsigned long long* d_has = nullptr;   // [has_cap] words, the keep bitmap's layout
    uint64_t has_cap = 0;
    uint32_t* d_rows = nullptr;            // one word: the resolution's count
    uint64_t rows = 0;                     // rows that have a value
    uint64_t resolved_at = ~0ull;          // the handle's mutation count and the version the resolution belongs to
    uint64_t resolved_version = 0;

    ~AttrColumn();
};

// Which rows a filter token keeps.  The consumers ask two things of a kind: whether its resolution leaves a keep bitmap
// (d_keep), and whether its position list waits for the first call that needs one (ensure_plist).
enum class FilterKind : uint8_t {
    Include,  // the rows whose id is in the set: the list at once, no bitmap
    Exclude,  // the rows whose id is NOT in the set: the bitmap, the list on demand
    Where,    // the rows whose attribute values pass 1..4 range clauses: the bitmap, the list on demand
};

struct WhereClause {
    std::shared_ptr<AttrColumn> column;  // the token's reference: the column outlives vl_index_attr_destroy
    int64_t lo, hi;
    bool negate;
    uint64_t version;  // the column version this token's resolution read
};

// An id filter of one single-GPU flat handle (vl_index_filter_create): the caller's ids, sorted and deduplicated, and -- resolved
// against the rows as they stood when the handle's mutation count was `resolved_at` -- the ascending storage positions of
// every row whose id is in the set.  A search that finds the count moved on resolves it again first.
// An EXCLUSION filter (vl_index_filter_create_excluding) qualifies the rows whose id is NOT in the set.
// Its resolution is the count m and a keep bitmap over storage positions; the position list is built by the first call
// that needs one after a resolution (ensure_plist), the masked single-query ladder never does.
// A PREDICATE filter (vl_index_filter_create_where, section 28) holds no ids: its clauses refer to attribute columns, its
// resolution is an exclusion filter's (m, the bitmap, the lazy list), and it is stale when a column's version moved too.
struct IdFilter {
    std::mutex mu;                         // guards everything below (taken after the index lock)
    int device = 0;
    FilterKind kind = FilterKind::Include;  // set at creation, never changes
    bool has_keep() const { return kind != FilterKind::Include; }
    bool lazy_list() const { return kind != FilterKind::Include; }
    std::vector<WhereClause> clauses;      // Where only
    std::vector<uint64_t> ids;             // sorted, unique
    unsigned long long* d_ids = nullptr;   // the same on the device
    uint32_t* d_counts = nullptr;          // [FILTER_COUNTS_MAX + 1] resolution scratch: per-chunk offsets, then m
    uint32_t* d_plist = nullptr;           // [plist_cap] positions of the qualifying rows, ascending
    uint64_t plist_cap = 0;
    bool plist_built = true;               // d_plist[0..m) belongs to this resolution (a lazy list: false until asked for)
    unsigned long long* d_keep = nullptr;  // has_keep() only: [keep_cap] words, bit p & 63 of word p >> 6 set iff row p qualifies
    uint64_t keep_cap = 0;
    uint64_t m = 0;                        // qualifying rows
    uint64_t resolved_at = ~0ull;          // the handle's mutation count the list belongs to (none yet)
    std::vector<uint32_t> h_plist;         // host copy of the list (the exact path maps its winners back), made on demand
    bool h_plist_valid = false;

    ~IdFilter();
};

// A group table of one single-GPU flat handle (vl_index_groups_create): the caller's (id, group key) pairs as a GroupPlan,
// and -- resolved like an id filter, with the same staleness rule -- the ascending positions of the rows that have a group
// (`rows`: an IdFilter over the table's ids) and group_of_row[position] for every row of the index.
struct GroupTable {
    IdFilter rows;                         // rows.mu guards everything here (taken after the index lock)
    std::vector<uint64_t> keys;            // dense group number -> the caller's key
    uint32_t* d_dense = nullptr;           // [rows.ids.size()] dense group number of each sorted id
    unsigned long long* d_keys = nullptr;  // [keys.size()]
    uint32_t* d_group_of_row = nullptr;    // [gor_cap] GROUP_NONE: the row has no group
    uint64_t gor_cap = 0;
    // the batched grouped search's keep bitmap of the table alone (bit p set iff row p has a group; section 26), built by the
    // first batch that needs it after a resolution
    unsigned long long* d_keep = nullptr;  // [keep_cap] words
    uint64_t keep_cap = 0;
    uint64_t keep_at = ~0ull;              // the mutation count the bitmap belongs to (none yet)

    ~GroupTable();
};

// A diversified search riding on a single search (search_mmr): how many candidates the selection returns, and lambda.
struct MmrReq {
    uint64_t k_out;
    double lambda;
};
int mmr_check_args(uint64_t k, uint64_t fetch_k, double lambda);  // VL_ERR_INVALID_ARG with a message, or OK

// Defined only by tests/native/derived_copies_audit.hip: reads the device copies, their watermarks and the host bookkeeping
// below to compare them with a from-scratch conversion after every mutation.  The library has no code of it.
class DerivedCopiesProbe;

class GpuFlatIndex {
    friend class DerivedCopiesProbe;

public:
    struct CoalesceReq {  // one caller waiting in search_coalesced()
        const double* query;
        uint64_t k;
        int metric;
        uint64_t* out_pos;
        uint64_t* out_ids;
        double* out_scores;
        uint64_t* out_n;
        int rc = 6;  // ERR_DEVICE until the pass answers it (a pass that dies must not read as success)
        int path = 0;
        std::string err = "coalesced pass ended without answering this request";
        bool done = false;
    };

    // FlatIndex::new(dim, Vec::new())
    static int create(uint64_t dim, int device, GpuFlatIndex** out);
    ~GpuFlatIndex();

    // trait VectorIndex (src/lib.rs:224-245)
    int add(uint64_t id, const double* values, uint64_t len);
    // values_on_device: `values` is device memory; src_device >= 0 names the GPU it lives on when that is not this
    // index's own (a multi-GPU handle replicating rows: hipMemcpyPeerAsync)
    int add_bulk(const uint64_t* ids, const double* values, uint64_t n, bool validate, bool values_on_device,
                 int src_device = -1);
    int remove(uint64_t id);  // `delete`
    // the same, reporting which storage positions went (descending) -- a sharded handle keeps a per-row table beside this index
    int remove_report(uint64_t id, std::vector<uint64_t>* removed_positions);
    // NEW (no reference counterpart): the state `for id in ids: delete(id)` leaves -- every row whose id is in the list goes,
    // the others keep their order -- reached with one walk over the ids and one pass over each device array (delete_plan.hpp,
    // k_move_rows), whatever n is.  Absent and repeated ids are no-ops.  removed_positions (may be null) receives the
    // positions that went, ascending; *out_rows their number.  DESIGN.md section 22.
    int remove_bulk(const uint64_t* ids, uint64_t n, std::vector<uint64_t>* removed_positions, uint64_t* out_rows);
    // bytes of the delete compaction buffer from now on (0: the default 64 MB; at least one row of the widest array); a
    // smaller buffer that exists is freed.  Small values make small indexes cross the plan's segment boundaries (tests).
    int set_delete_bounce(uint64_t bytes);
    // the last remove_bulk on this handle: rows removed, rows moved, direct launches, bounced segments, bytes written to
    // device memory, microseconds from the first launch to the end of the synchronisation
    void last_delete(uint64_t out[6]) const
    {
        for (int i = 0; i < 6; ++i) out[i] = last_delete_[i].load(std::memory_order_relaxed);
    }
    // NEW (no reference counterpart): replaces the values of the FIRST row carrying `id` (get_vector's rule) in place:
    // length, row order, ids_, mutations_ and every token's resolved state stay as they are.  ERR_NOT_FOUND: no such row.
    int update(uint64_t id, const double* values, uint64_t len);
    // the state the loop `contains(ids[i]) ? update(ids[i], values_i) : (insert_missing ? add(ids[i], values_i) : fail)`
    // leaves (update_plan.hpp): a repeated id keeps its last values, an absent id is appended once.  A refusal
    // (ERR_NOT_FOUND: an absent id without insert_missing) is decided before any device write.  The rewritten rows go up in
    // position-sorted chunks through the bounce buffer (set_delete_bounce sizes it), k_update_rows rewrites master, slab,
    // inv_norm and flags, k_update_copies the rows of each lazy copy below its watermark; appended rows take the add
    // path.  *out_updated = distinct rows rewritten, *out_inserted = rows appended (either may be null).  DESIGN.md section 25.
    int update_bulk(const uint64_t* ids, const double* values, uint64_t n, bool insert_missing, uint64_t* out_updated,
                    uint64_t* out_inserted);
    // the last update / update_bulk on this handle (all zero if it did nothing): rows rewritten, rows appended, rows
    // rewritten in the row-major bf16 copy, in the fragment-major one, in the int8 copy, staging chunks, microseconds from
    // the first launch to the end of the last synchronisation
    void last_update(uint64_t out[7]) const
    {
        for (int i = 0; i < 7; ++i) out[i] = last_update_[i].load(std::memory_order_relaxed);
    }
    bool contains(uint64_t id) const;                       // O(1) after the first call (the duplicate-id table)
    int find_first(uint64_t id, uint64_t* out_pos) const;   // first row with that id (get_vector's rule); ERR_NOT_FOUND
    int get_row_at(uint64_t pos, double* out) const;
    int search(const double* query, uint64_t q_len, uint64_t k, int metric, uint64_t* out_pos,
               uint64_t* out_ids, double* out_scores, uint64_t* out_n) const;
    // NEW (no reference counterpart): nq independent searches sharing slab passes; outputs are
    // [nq, k] with row stride k.
    int search_batch(const double* queries, uint64_t nq, uint64_t q_len, uint64_t k, int metric, uint64_t* out_pos,
                     uint64_t* out_ids, double* out_scores, uint64_t* out_n) const;
    // NEW: search_batch with the queries already in device memory of this index's GPU (embeddings computed there): the
    // MFMA batch path stages them with a kernel -- no host staging, no PCIe copy of the queries; whatever that path does
    // not serve (Manhattan, one query, small indexes, queries it cannot certify) is copied to the host and answered there.
    int search_batch_device(const double* d_queries, uint64_t nq, uint64_t q_len, uint64_t k, int metric, uint64_t* out_pos,
                            uint64_t* out_ids, double* out_scores, uint64_t* out_n) const;
    // A row shard's answer written straight into the DEVICE planes of its exchange record (shard.hpp; `record` = the
    // record's first word in this GPU's memory, stride ks = k): the finalize kernel fills count / score / global position /
    // id of every query it certifies, the few it cannot are redone through the host paths and their slices patched.  Queries
    // on the host (queries_on_device = false) or in this GPU's memory.  *handled = false (and nothing written): this batch
    // does not take the MFMA filter (Manhattan, one query, a small or empty shard, out-of-domain rows, k > 60 ...) -- the
    // caller then builds the record on the host as before.  Word 0..3 of the record (status, len, dim) are the caller's.
    int search_batch_to_record(const double* queries, bool queries_on_device, uint64_t nq, uint64_t q_len, uint64_t ks,
                               int metric, uint64_t row_offset, unsigned long long* d_record, bool* handled) const;
    // NEW (no reference counterpart): search restricted to the rows whose id is in a set.  The answer is exactly what
    // FlatIndex::search returns on a FlatIndex holding only those rows, in their storage order.  A filter is a token of this
    // handle (never 0, never reused); ids may be unsorted and repeat; ids the index does not hold are ignored.
    // exclude: the rows whose id is NOT in the set qualify (n_ids = 0 keeps every row; an id added later is excluded then)
    int filter_create(const uint64_t* ids, uint64_t n_ids, uint64_t* out_token, uint64_t* out_rows, bool exclude = false);
    // NEW (no reference counterpart): attribute columns (id -> int64) and filter tokens that keep the
    // rows whose values pass 1..4 ANDed range clauses, resolved on the device (where.hip).  Column tokens come from the
    // filters' counter.  attr_set upserts pairs (attr_plan_merge); a refusal leaves the column as it was.
    int attr_create(AttrPlan&& plan, uint64_t* out_token, uint64_t* out_rows);  // the caller's pairs, planned (attr_plan.hpp)
    int attr_set(uint64_t attr, const uint64_t* ids, const int64_t* values, uint64_t n);
    int attr_rows(uint64_t attr, uint64_t* out_rows) const;  // rows that have a value now
    int attr_destroy(uint64_t attr);                          // tokens made from the column keep it alive and keep working
    struct WhereSpec {
        uint64_t attr;
        int64_t lo, hi;
        bool negate;
    };
    // a row qualifies iff for every clause it has a value v in that column and (lo <= v && v <= hi) != negate
    int filter_create_where(const WhereSpec* clauses, uint64_t n_clauses, uint64_t* out_token, uint64_t* out_rows);
    // How a single search under a predicate token runs (where_plan.hpp).  0 ("auto", the default): the masked ladder when
    // its byte estimate is below the list's.  1: the position list.  2: the ladder wherever its conditions hold.
    void set_where_route(int mode) { where_route_.store(mode); }
    int where_route() const { return where_route_.load(); }
    // the route of the last single predicate-filtered search (0 list, 1 masked ladder), its m, and the predicate and
    // column resolutions on this handle so far
    void last_where(uint64_t out[4]) const
    {
        for (int i = 0; i < 4; ++i) out[i] = last_where_[i].load(std::memory_order_relaxed);
    }
    int filter_rows(uint64_t token, uint64_t* out_rows) const;  // resolves the filter again if rows changed since
    int filter_destroy(uint64_t token);
    // for the HNSW graph layered on this row store (hnsw_index.cpp): the filter's ascending position list on the device,
    // resolved again first if rows changed since.  Valid while the caller holds *keep and keeps rows from being added.
    int filter_positions(uint64_t token, std::shared_ptr<IdFilter>* keep, const uint32_t** d_plist, uint64_t* m) const;
    int search_filtered(uint64_t token, const double* query, uint64_t q_len, uint64_t k, int metric, uint64_t* out_pos,
                        uint64_t* out_ids, double* out_scores, uint64_t* out_n) const;
    // NEW: nq filtered searches against one index state, one filter for all of them (n_filters == 1) or one per query
    // (n_filters == nq; tokens may repeat).  Row i of the [nq, out_stride] outputs is exactly search_filtered(tokens[i], queries
    // + i * q_len, ..., k)'s answer; k <= out_stride.  The jobs that may take the fast path share launches of
    // k_scan_subset_jobs (subset_batch_plan.hpp) and one finalize launch each; the rest, and what a launch could not certify,
    // go through search_subset.  Returns the status of the lowest-numbered failing query; out_n is 0 from that query on.
    int search_batch_filters(const uint64_t* tokens, uint64_t n_filters, const double* queries, uint64_t nq, uint64_t q_len,
                             uint64_t k, int metric, uint64_t out_stride, uint64_t* out_ids, double* out_scores,
                             uint64_t* out_n) const;
    // the last search_batch_filters on this handle: jobs answered by a batched launch, jobs handed to the single filtered
    // search before any launch, jobs a batched launch could not certify (redone on the exact kernels), batched scan launches
    void last_filtered_batch(uint64_t* batched, uint64_t* single, uint64_t* exact, uint64_t* launches) const
    {
        if (batched) *batched = last_fbatch_[0].load(std::memory_order_relaxed);
        if (single) *single = last_fbatch_[1].load(std::memory_order_relaxed);
        if (exact) *exact = last_fbatch_[2].load(std::memory_order_relaxed);
        if (launches) *launches = last_fbatch_[3].load(std::memory_order_relaxed);
    }
    // How search_batch_filters answers queries under EXCLUSION tokens (masked_batch_plan.hpp).  0: with
    // the jobs kernel, like include tokens.  1: the eligible ones with the mask-aware MFMA pass.  2 ("auto", the default):
    // the pass when its estimated time is below the jobs kernel's.
    void set_masked_batch(int mode) { masked_batch_.store(mode); }
    int masked_batch() const { return masked_batch_.load(); }
    // the last search_batch_filters on this handle: queries sent to the masked MFMA pass, those it certified, those it
    // handed back (they are counted by last_filtered_batch like any other job), its launch sequences, and the position
    // lists of exclusion tokens the call had to build (0: the pass answered every query of those tokens)
    void last_masked_batch(uint64_t* routed, uint64_t* certified, uint64_t* redone, uint64_t* sequences, uint64_t* lists_built) const
    {
        uint64_t* out[5] = {routed, certified, redone, sequences, lists_built};
        for (int i = 0; i < 5; ++i)
            if (out[i]) *out[i] = last_mbatch_[i].load(std::memory_order_relaxed);
    }
    // NEW (no reference counterpart): every row whose score is >= min_score -- the longest prefix of FlatIndex::search(q, len,
    // metric) with score >= min_score, over the filter's rows when token != 0.  *out_total = rows that qualify, always;
    // min(total, out_capacity) entries are written (out_capacity = 0: count only, outputs may be null).
    int search_range(uint64_t token, const double* query, uint64_t q_len, double min_score, int metric, uint64_t out_capacity,
                     uint64_t* out_pos, uint64_t* out_ids, double* out_scores, uint64_t* out_n, uint64_t* out_total) const;
    // NEW (no reference counterpart): nq range searches against one index state; row i of the [nq, out_stride] outputs is
    // exactly search_range(token, queries + i * q_len, q_len, min_scores[i], metric, out_stride, ...).  Returns the status of
    // the lowest-index failing query.  DESIGN.md section 17.
    int search_range_batch(uint64_t token, const double* queries, uint64_t nq, uint64_t q_len, const double* min_scores, int metric,
                           uint64_t out_stride, uint64_t* out_ids, double* out_scores, uint64_t* out_n, uint64_t* out_total) const;
    // the last search_range_batch on this handle: queries answered by the MFMA pass + device tail, by the single-query fast
    // route (k_scan_range), by the exact route; and the largest candidate count the MFMA pass reported for a query it kept
    void last_range_batch(uint64_t* mfma, uint64_t* single, uint64_t* exact, uint64_t* max_candidates) const
    {
        if (mfma) *mfma = last_rbatch_[0].load(std::memory_order_relaxed);
        if (single) *single = last_rbatch_[1].load(std::memory_order_relaxed);
        if (exact) *exact = last_rbatch_[2].load(std::memory_order_relaxed);
        if (max_candidates) *max_candidates = last_rbatch_[3].load(std::memory_order_relaxed);
    }
    // NEW (no reference counterpart): maximal marginal relevance over C = FlatIndex::search(q, fetch_k, metric) on the whole
    // index (token 0) or the filter's rows: sel[0] = C[0], then greedily the candidate maximising
    // lambda * score - (1 - lambda) * (largest reference similarity to anything chosen), ties to the better-ranked one.
    // min(k, |C|, out_capacity) entries in selection order, scores = the candidates' reference scores.
    int search_mmr(uint64_t token, const double* query, uint64_t q_len, uint64_t k, uint64_t fetch_k, double lambda, int metric,
                   uint64_t out_capacity, uint64_t* out_pos, uint64_t* out_ids, double* out_scores, uint64_t* out_n) const;
    // NEW (no reference counterpart): nq diversified searches against one index state; row i of the [nq, out_stride] outputs
    // and out_n[i] are exactly search_mmr(token, queries + i * q_len, q_len, k, fetch_k, lambda, metric, out_stride, ...).
    // Eligible batches (mmr_batch_plan.hpp) share passes of the bf16 MFMA filter, followed per query by the rescoring and
    // the rank / similarity / selection stage (mmr.hip); whatever a pass does not settle, and every batch that is not
    // eligible, runs the single search's body under the same lock.  Returns the status of the lowest-index failing query.
    // DESIGN.md section 27.
    int search_mmr_batch(uint64_t token, const double* queries, uint64_t nq, uint64_t q_len, uint64_t k, uint64_t fetch_k,
                         double lambda, int metric, uint64_t out_stride, uint64_t* out_ids, double* out_scores,
                         uint64_t* out_n) const;
    // 0: always the loop.  1: the pass whenever the batch is eligible.  2 ("auto", the default): when its estimate is lower.
    void set_mmr_batch(int mode) { mmr_batch_.store(mode); }
    int mmr_batch() const { return mmr_batch_.load(); }
    // the last search_mmr_batch on this handle: queries sent to the pass, those it settled, those it handed back to the
    // single search, its launch sequences; all zero when the call looped
    void last_mmr_batch(uint64_t* routed, uint64_t* settled, uint64_t* handed_back, uint64_t* sequences) const
    {
        uint64_t* out[4] = {routed, settled, handed_back, sequences};
        for (int i = 0; i < 4; ++i)
            if (out[i]) *out[i] = last_mmrbatch_[i].load(std::memory_order_relaxed);
    }
    // NEW (no reference counterpart): the best row of each of the best k groups.  A group table maps
    // ids to caller-chosen u64 group keys; rows whose id it does not hold take no part.  With S = the FlatIndex of the rows
    // that have a group (and, token != 0, pass the filter) in storage order, the answer is search(q, len(S)) on S walked from
    // the front, a row emitted iff no earlier row has its group key, until k rows are out.
    int groups_create(GroupPlan&& plan, uint64_t* out_token, uint64_t* out_rows);  // the caller's pairs, planned (group_plan.hpp)
    int groups_rows(uint64_t groups, uint64_t* out_rows, uint64_t* out_distinct) const;  // resolves again if rows changed since
    int groups_destroy(uint64_t groups);
    int search_grouped(uint64_t groups, uint64_t token, const double* query, uint64_t q_len, uint64_t k, int metric,
                       uint64_t out_capacity, uint64_t* out_group_keys, uint64_t* out_pos, uint64_t* out_ids, double* out_scores,
                       uint64_t* out_n) const;
    // NEW (no reference counterpart): nq grouped searches against one index state; row i of the [nq, out_stride] outputs and
    // out_n[i] are exactly search_grouped(groups, token, queries + i * q_len, q_len, k, metric, out_stride, ...).  Eligible
    // batches (grouped_batch_plan.hpp) share passes of the bf16 MFMA filter, followed per query by the rescoring and the
    // rank-and-collapse stage; whatever a pass does not settle, and every batch that is not eligible, runs the single
    // search's body under the same lock.  Returns the status of the lowest-index failing query.  DESIGN.md section 26.
    int search_grouped_batch(uint64_t groups, uint64_t token, const double* queries, uint64_t nq, uint64_t q_len, uint64_t k,
                             int metric, uint64_t out_stride, uint64_t* out_group_keys, uint64_t* out_ids, double* out_scores,
                             uint64_t* out_n) const;
    // 0: always the loop.  1: the pass whenever the batch is eligible.  2 ("auto", the default): when its estimate is lower.
    void set_grouped_batch(int mode) { grouped_batch_.store(mode); }
    int grouped_batch() const { return grouped_batch_.load(); }
    // the last search_grouped_batch on this handle: queries sent to the pass, those it settled, those it handed back to the
    // single search, its launch sequences; all zero when the call looped
    void last_grouped_batch(uint64_t* routed, uint64_t* settled, uint64_t* handed_back, uint64_t* sequences) const
    {
        uint64_t* out[4] = {routed, settled, handed_back, sequences};
        for (int i = 0; i < 4; ++i)
            if (out[i]) *out[i] = last_gbatch_[i].load(std::memory_order_relaxed);
    }
    uint64_t len() const;
    bool is_empty() const { return len() == 0; }
    uint64_t dimension() const { return dim_; }
    int get_vector(uint64_t id, double* out) const;
    int max_id(uint64_t* out) const;

    int clone(GpuFlatIndex** out) const;
    int reserve(uint64_t n_rows);
    // forget the rows at positions >= n_rows (host bookkeeping only, cannot fail): how a multi-GPU handle takes back the
    // part of a bulk add that another part could not complete
    void truncate(uint64_t n_rows);
    int export_rows(uint64_t* out_ids, double* out_values) const;
    int hnsw_distances(const double* query, uint64_t q_len, int metric, const uint64_t* positions, uint64_t m,
                       uint64_t* out) const;

    // storage access for the HNSW graph layered on top of this row store (hnsw_index.cpp)
    const double* device_master() const { return d_master_; }
    const float* device_slab() const { return d_slab_; }
    const float* device_inv_norm() const { return d_inv_norm_; }
    uint32_t slab_ld() const { return ld_; }
    uint64_t capacity() const { return cap_; }

    void force_path(int p) { force_path_.store(p); }
    // Which copies a single query scans before the f32 slab (single_filter.hpp).  0: the f32 slab only.  1: the bf16 copy
    // first, always (half the bytes; switches itself off for good once more than a third of 64+ tries failed to certify).
    // 2 ("auto", the default): the ladder int8 -> bf16 -> f32: the int8 copy (a quarter of the bytes) when the f32 slab is
    // at least SINGLE_FILTER_I8_MIN_BYTES (VL_SINGLE_FILTER_I8_MIN_MB at create), the bf16 copy when it is at least
    // SINGLE_FILTER_MIN_BYTES (VL_SINGLE_FILTER_MIN_MB), each paused by its own AutoFilterWindow while it fails to
    // certify.  3: the int8 copy first, always (cosine and dot; mode 1's one-way rule), then the f32 slab.
    void set_single_filter(int mode)
    {
        single_filter_.store(mode);
        bf16_tries_.store(0);
        bf16_fails_.store(0);
        i8_tries_.store(0);
        i8_fails_.store(0);
        auto_window_.reset();
        i8_window_.reset();
        for (auto* c : {&mask_bf16_tries_, &mask_bf16_fails_, &mask_i8_tries_, &mask_i8_fails_}) c->store(0);
        mask_bf16_window_.reset();
        mask_i8_window_.reset();
        auto_unavailable_.store(false);
        i8_unavailable_.store(false);
    }
    int single_filter() const { return single_filter_.load(); }
    void set_single_filter_min_bytes(uint64_t b) { auto_min_bytes_ = b; }
    void set_single_filter_i8_min_bytes(uint64_t b) { i8_min_bytes_ = b; }
    // Group concurrent single-query search() calls into shared slab passes (coalescer.hpp, search_coalesced()).
    // max_batch <= 1 turns it off.  window_us: how long a lone caller waits for company.  create() turns it on with
    // (COALESCE_DEFAULT_BATCH, 0) unless VL_COALESCE=0.
    void set_coalescing(int max_batch, int window_us) { co_.configure(max_batch, window_us, (int)MFMA_MAX_BATCH); }
    void coalesce_stats(uint64_t* batches, uint64_t* queries) const { co_.stats(batches, queries); }
    // adaptive: 1 / 0 switch the leader's adaptive gather (coalescer.hpp) on / off, -1 leaves it; waits, waited_us: passes whose
    // leader waited for its peers and the time spent waiting, since creation
    void coalesce_gather(int adaptive, uint64_t* waits, uint64_t* waited_us) const
    {
        if (adaptive >= 0) co_.set_adaptive(adaptive != 0);
        co_.gather_stats(waits, waited_us);
    }
    void profile_enable(bool on);
    void profile_read(uint64_t* n, double* ms, uint64_t* bytes);
    // which k_scan instantiation (G * 10000 + VPL * 100 + U; negative: the generic kernel's G), on how many workgroups,
    // the last single f32 scan used, and whether its query travelled in the kernel arguments
    void last_scan(int* variant, int* grid, int* qarg) const
    {
        if (variant) *variant = last_scan_variant_.load();
        if (grid) *grid = last_scan_grid_.load();
        if (qarg) *qarg = last_scan_qarg_.load();
    }
    // the batch filter's last launch sequence on this handle: {K steps of 16, metric, query chunks, workgroups per chunk of
    // the last pass-1 stage, pass-1 stages, 32-row blocks sampled}; all zero before the first MFMA batch
    void last_filter(int out[6]) const
    {
        for (int i = 0; i < 6; ++i) out[i] = last_filter_[i].load(std::memory_order_relaxed);
    }
    int device() const { return device_; }

private:
    GpuFlatIndex(uint64_t dim, int device);
    int ensure_capacity(uint64_t rows);  // caller holds the unique lock
    int ingest_range(uint64_t first, uint64_t n);
    // add_bulk's body; the caller holds the unique lock and has set the device
    int add_bulk_locked(const uint64_t* ids, const double* values, uint64_t n, bool validate, bool values_on_device, int src_device);
    int remove_position(uint64_t pos);
    void rebuild_id_counts() const;
    Workspace* acquire_ws() const;
    void release_ws(Workspace* ws) const;
    int prepare_ws(Workspace* ws) const;
    // What every read-side entry point shares.  A new search mode writes its argument rules and its
    // *_locked body, nothing else.
    class WsLease;  // a borrowed workspace: hipSetDevice + acquire_ws; drains the stream if the call failed, then gives it back
    int lock_for_query(int metric, uint64_t q_len, std::shared_lock<RwLock>* lk) const;  // the metric, then mu_ shared, then the length
    int dim_mismatch(uint64_t q_len) const;  // records it; VL_ERR_DIM_MISMATCH
    // mu_ held (shared): leases a workspace, resolves t and f (either may be null) if rows changed since, runs body(ws) as one
    // of the handle's searches in flight
    template <typename Body>
    int run_search(GroupTable* t, IdFilter* f, Body&& body, bool need_list = true) const;
    // takes f->mu; need_list: the caller reads f->d_plist (an exclusion filter builds it then, once per resolution)
    int resolve_if_stale(Workspace* ws, IdFilter* f, bool need_list = true) const;
    int ensure_plist(Workspace* ws, IdFilter* f) const;  // mu_ held, f->mu held, f resolved
    int resolve_if_stale(Workspace* ws, GroupTable* t) const;  // takes t->rows.mu
    int account_profile(Workspace* ws, uint64_t bytes, uint64_t passes = 1) const;  // the scan between ws->ev0 and ws->ev1
    void note_scan(int variant, int grid, bool qarg) const
    {
        last_scan_variant_.store(variant, std::memory_order_relaxed);
        last_scan_grid_.store(grid, std::memory_order_relaxed);
        last_scan_qarg_.store(qarg ? 1 : 0, std::memory_order_relaxed);
    }
    int search_direct(const double* query, uint64_t q_len, uint64_t k, int metric, uint64_t* out_pos, uint64_t* out_ids,
                      double* out_scores, uint64_t* out_n) const;
    int search_coalesced(const double* query, uint64_t q_len, uint64_t k, int metric, uint64_t* out_pos,
                         uint64_t* out_ids, double* out_scores, uint64_t* out_n) const;
    void run_coalesced(std::vector<CoalesceReq*>& batch) const;
    // skip_bf16: the query already failed a bf16 filter's certification (an MFMA batch straggler): neither the int8 nor the
    // bf16 stage, straight to k_scan
    // mmr != nullptr (search_mmr): k_eff = the candidates to fetch; the outputs receive mmr->k_out selected entries
    // mask != nullptr (search_filtered with an exclusion filter): the ladder runs its masked launchers over the whole slab,
    // certifies against the mask's m rows with switches and counters of its own, and returns MASK_UNCERTIFIED -- with
    // nothing written -- where no stage certified: the caller then takes the list route.  k_eff <= mask->m.
    static constexpr int MASK_UNCERTIFIED = -1000;  // never leaves flat_index.cpp
    int search_locked(Workspace* ws, const double* query, uint64_t k_eff, int metric, uint64_t* out_pos,
                      uint64_t* out_ids, double* out_scores, uint64_t* out_n, bool skip_fast, bool skip_bf16 = false,
                      const MmrReq* mmr = nullptr, const IdFilter* mask = nullptr) const;
    // the selection's two launches behind a search's last kernel (ws->h_result receives the answer; seq != 0: stamped)
    int mmr_tail(Workspace* ws, int metric, const MmrReq& m, MmrSource src, uint32_t seq) const;
    int mmr_take(Workspace* ws, const MmrReq& m, uint64_t* out_pos, uint64_t* out_ids, double* out_scores,
                 uint64_t* out_n) const;
    // masked: the masked ladder's own windows and counters (the mode and the floors are shared)
    bool bf16_first(uint64_t n, bool masked = false) const;        // does this single search try the bf16 filter (after the int8 one)
    void bf16_outcome(bool certified, bool masked = false) const;  // records one try of the bf16 filter
    bool i8_first(uint64_t n, bool masked = false) const;          // does this single search try the int8 filter first
    void i8_outcome(bool certified, bool masked = false) const;    // records one try of the int8 filter
    // plist != nullptr: the n rows are plist[0..n) (a filter's subset) and pos[] returns indices into that list
    // mmr != nullptr: the selection runs behind the ranking and pos / scores stay untouched (mmr_take reads the answer)
    int run_exact(Workspace* ws, int metric, uint64_t n, uint64_t k_eff, std::vector<uint32_t>* pos,
                  std::vector<double>* scores, const uint32_t* plist = nullptr, const MmrReq* mmr = nullptr) const;
    int find_filter(uint64_t token, std::shared_ptr<IdFilter>* out) const;  // VL_ERR_INVALID_ARG with a message: no such token
    int resolve_filter(Workspace* ws, IdFilter* f) const;  // mu_ held (shared or unique), f->mu held
    bool filter_stale(const IdFilter* f) const;            // likewise: rows moved, or (a predicate token) a column's version did
    int resolve_where(Workspace* ws, IdFilter* f) const;   // resolve_filter's body for a predicate token
    int resolve_attr(Workspace* ws, AttrColumn* c) const;  // mu_ held, c->mu held
    int upload_attr(AttrColumn* c) const;                  // c->plan -> the device; c->mu held or c not yet shared
    int find_attr(uint64_t token, std::shared_ptr<AttrColumn>* out) const;
    int where_first_stage(uint64_t n, int metric) const;   // WHERE_STAGE_*: the masked ladder's first stage as things stand
    // exact_only: the fast path already failed to certify this (query, filter) in a batched launch: straight to the exact kernels
    int search_subset(Workspace* ws, IdFilter* f, const double* query, uint64_t k_eff, int metric, uint64_t* out_pos,
                      uint64_t* out_ids, double* out_scores, uint64_t* out_n, const MmrReq* mmr = nullptr,
                      bool exact_only = false) const;  // mu_ held (shared), f resolved
    int search_range_locked(Workspace* ws, IdFilter* f, const double* query, double min_score, int metric, uint64_t out_capacity,
                            uint64_t* out_pos, uint64_t* out_ids, double* out_scores, uint64_t* out_n,
                            uint64_t* out_total) const;  // mu_ held (shared), f resolved (nullptr: the whole index)
    int find_groups(uint64_t token, std::shared_ptr<GroupTable>* out) const;
    int resolve_groups(Workspace* ws, GroupTable* t) const;  // mu_ held (shared or unique), t->rows.mu held
    // mu_ held (shared), t resolved, f resolved (nullptr: no filter)
    int search_grouped_locked(Workspace* ws, const GroupTable* t, const IdFilter* f, const double* query, uint64_t k, int metric,
                              uint64_t out_capacity, uint64_t* out_group_keys, uint64_t* out_pos, uint64_t* out_ids,
                              double* out_scores, uint64_t* out_n) const;
    // the MFMA route of search_range_batch (mu_ held, whole index): done[qi] is set for every query answered here
    int search_range_batch_mfma(Workspace* ws, const double* queries, uint64_t nq, const double* min_scores, int metric,
                                uint64_t out_stride, uint64_t* out_ids, double* out_scores, uint64_t* out_n, uint64_t* out_total,
                                std::vector<uint8_t>* done, uint64_t* max_candidates) const;
    int wait_result(Workspace* ws, uint32_t seq) const;
    int ensure_i8_slab() const;  // lazily builds the int8 copy the single-query int8 filter streams
    int ensure_bf16_slab(bool frag_major) const;  // lazily builds the bf16 slab (row-major, or MFMA fragment order) a filter streams
    int ensure_mfma_scratch(Workspace* ws) const;
    int search_batch_locked(const double* queries, uint64_t nq, uint64_t q_len, uint64_t k, int metric, uint64_t* out_pos,
                            uint64_t* out_ids, double* out_scores, uint64_t* out_n) const;  // mu_ held (shared)
    // Per-query descriptor of a masked batch (exclusion tokens): sequence query j is the caller's
    // query qidx[j] (host queries only) under the keep bitmap keep[j] (a device pointer), which keeps m[j] > 0 rows; it asks
    // for k[j] = min(k, m[j]) rows.  Outputs and `done` are indexed by j, at stride k.
    struct MaskedQueries {
        const uint32_t* qidx;
        const unsigned long long* const* keep;
        const uint32_t* m;
        const uint32_t* k;
    };
    // A batched grouped search riding on the sequence pipeline: k_batch_rank_collapse takes the
    // rank / emit launch's place and settled queries are unpacked as (group key, id, score) rows, out_stride apart.  S has m
    // rows: every row of the index (masked == nullptr) or the rows under the one bitmap every query of `masked` names.
    // Host queries only; out_pos / out_n / done as ever, out_ids and out_scores at stride out_stride like out_keys.
    struct GroupedReq {
        const GroupTable* table;
        uint64_t m;
        uint64_t out_stride;
        uint64_t* out_keys;
    };
    // A batched diversified search riding on the sequence pipeline: k_mmr_batch_rank and
    // k_mmr_batch_select take the rank / emit launch's place and settled queries are unpacked as (id, score) rows in selection
    // order, out_stride apart.  S has m rows: every row of the index (masked == nullptr) or the rows under the one bitmap every
    // query of `masked` names.  n = min(fetch_k, m) <= KFAST_MAX candidates, k_out = min(k, n, out_stride) >= 1 chosen.
    struct MmrBatchReq {
        uint64_t m;
        uint64_t n;
        uint64_t k_out;
        double lambda;
        uint64_t out_stride;
    };
    int search_batch_mfma(Workspace* ws, const double* queries, const double* d_queries, uint64_t nq, uint64_t k,
                          uint64_t k_eff, int metric, uint64_t* out_pos, uint64_t* out_ids, double* out_scores,
                          uint64_t* out_n, std::vector<uint8_t>* done,
                          const ShardRecordSink* sink = nullptr,  // queries on the host, or d_queries on the device
                          const MaskedQueries* masked = nullptr, uint64_t* n_sequences = nullptr,
                          const GroupedReq* grouped = nullptr, const MmrBatchReq* mmr = nullptr) const;
    // the locked body of search_mmr: mu_ held (shared), the filter resolved with its position list, n != 0, k_cap != 0
    int search_mmr_locked(Workspace* ws, IdFilter* f, const double* query, uint64_t k_cap, uint64_t fetch_k, double lambda,
                          int metric, uint64_t* out_pos, uint64_t* out_ids, double* out_scores, uint64_t* out_n) const;
    // the keep bitmap of S = the table's rows under f (nullptr: the table alone, cached on the table) and |S|; mu_ held,
    // t and f resolved.  No position list is built.
    int grouped_keep_bits(Workspace* ws, GroupTable* t, IdFilter* f, const unsigned long long** keep, uint64_t* m) const;
    int ensure_device_ids() const;  // lazily uploads the position -> id table (what a device-written exchange record needs)

    const uint64_t dim_;
    const uint32_t ld_;  // slab row stride in floats: dim rounded up to 4 (16-byte vector loads)
    const int device_;

    mutable RwLock mu_;  // search: shared; add/delete: unique
    // device storage
    double* d_master_ = nullptr;  // [cap, dim] f64: exact rows
    float* d_slab_ = nullptr;     // [cap, ld]  f32: what the scan streams
    float* d_inv_norm_ = nullptr; // [cap]      f32: 1/|row|, 0 for zero rows
    uint8_t* d_flags_ = nullptr;  // [cap]
    mutable void* d_slab16_ = nullptr;     // [cap, ldb] bf16: candidate filter of the MFMA batch path (lazy)
    mutable float* d_norm16_ = nullptr;    // [cap] f32 |row| (the bf16 slab rows are unit-normalised)
    mutable float* d_sqnorm_ = nullptr;    // [cap] f32 |row|^2 for the GEMM-form Euclidean key (with d_slab16_)
    mutable uint64_t slab16_rows_ = 0;     // rows converted so far (== len() once built)
    mutable void* d_slab16f_ = nullptr;    // the same rows in MFMA fragment order: what k_mfma_rows streams (lazy; dims <= 384)
    mutable uint64_t slab16f_rows_ = 0;
    // The int8 copy (rebuilt on demand like the row-major bf16 one; never cloned, exported or persisted): [cap, ldb]
    // offset-binary bytes of the unit rows, per row the (s, r) pair of k_rows_i8 and |row| (f32).  All three or none.
    mutable void* d_slab8_ = nullptr;
    mutable float* d_sr8_ = nullptr;     // [cap][2]
    mutable float* d_norm8_ = nullptr;   // [cap]
    mutable uint64_t slab8_rows_ = 0;    // rows converted so far
    mutable std::mutex bf16_mu_;         // (also guards the int8 copy)
    mutable unsigned long long* d_ids_ = nullptr;  // [d_ids_cap_] position -> id on the device (lazy: row-sharded batches only)
    mutable uint64_t d_ids_cap_ = 0, d_ids_rows_ = 0;  // rows uploaded so far (a delete rewinds it like the bf16 copies)
    IngestStats* d_stats_ = nullptr;
    uint64_t cap_ = 0;  // rows every array holds (the minimum of the four below)
    uint64_t cap_master_ = 0, cap_slab_ = 0, cap_inv_ = 0, cap_flags_ = 0;
    hipStream_t mut_stream_ = nullptr;
    void* d_bounce_ = nullptr;  // delete compaction buffer; an update's staging buffer
    size_t bounce_bytes_ = 0;
    size_t bounce_want_ = 0;    // set_delete_bounce: what remove_bulk plans with and allocates (0: BOUNCE_BYTES)

    // host bookkeeping
    std::vector<uint64_t> ids_;        // position -> id (insertion order)
    uint64_t mutations_ = 0;           // changes of ids_ or of the row order so far (an id filter's staleness test)
    std::vector<uint8_t> row_flags_;   // position -> ROW_* flags
    uint64_t n_out_of_domain_ = 0;
    double max_row_norm_ = 0.0;        // upper bound over in-domain rows ever stored
    mutable std::unordered_map<uint64_t, uint32_t> id_counts_;  // id -> multiplicity (lazy)
    mutable bool id_counts_valid_ = true;

    // workspace pool
    static WorkspacePool* attach_pool(int device, uint64_t dim);
    static void detach_pool(int device, uint64_t dim);
    WorkspacePool* ws_pool_ = nullptr;

    mutable Coalescer<CoalesceReq> co_;

    mutable std::mutex filters_mu_;  // the filter table; never held while an index lock or a filter's mutex is taken
    std::unordered_map<uint64_t, std::shared_ptr<IdFilter>> filters_;
    std::unordered_map<uint64_t, std::shared_ptr<GroupTable>> groups_;  // under filters_mu_ as well; tokens share the filters' counter
    std::unordered_map<uint64_t, std::shared_ptr<AttrColumn>> attrs_;   // likewise
    std::atomic<int> where_route_{0};  // WHERE_ROUTE_AUTO
    mutable std::atomic<uint64_t> last_where_[4] = {};

    std::atomic<int> force_path_{0};
    std::atomic<int> single_filter_{FILTER_AUTO};
    mutable std::atomic<uint64_t> bf16_tries_{0}, bf16_fails_{0};  // mode 1
    mutable std::atomic<uint64_t> i8_tries_{0}, i8_fails_{0};      // mode 3
    // auto: below this f32 slab size back-to-back searches find the slab in the 256 MiB Infinity Cache and the f32 scan
    // is as fast as the bf16 one (profiles/single_filter_crossover.jsonl)
    static constexpr uint64_t SINGLE_FILTER_MIN_BYTES = 512ull << 20;
    uint64_t auto_min_bytes_ = SINGLE_FILTER_MIN_BYTES;
    mutable AutoFilterWindow auto_window_;
    mutable std::atomic<bool> auto_unavailable_{false};  // the bf16 copy could not be allocated: auto stays on f32
    // auto's int8 stage: its own floor (VL_SINGLE_FILTER_MIN_MB does not lower it).  Below 1 GiB the copy -- a fourth
    // image of the data, +0.25 x the f32 slab -- would save a few tens of us at most (profiles/single_filter_i8_crossover.jsonl).
    static constexpr uint64_t SINGLE_FILTER_I8_MIN_BYTES = 1024ull << 20;
    uint64_t i8_min_bytes_ = SINGLE_FILTER_I8_MIN_BYTES;
    mutable AutoFilterWindow i8_window_;
    mutable std::atomic<bool> i8_unavailable_{false};  // the int8 copy could not be allocated: auto goes on to bf16
    // the masked ladder's (an exclusion filter's single searches) windows and mode-1 / mode-3 counters: what it certifies
    // depends on what was excluded, so it neither reads nor feeds the unfiltered ladder's
    mutable AutoFilterWindow mask_bf16_window_, mask_i8_window_;
    mutable std::atomic<uint64_t> mask_bf16_tries_{0}, mask_bf16_fails_{0}, mask_i8_tries_{0}, mask_i8_fails_{0};
    std::atomic<bool> profile_{false};
    // single searches in flight on this handle: up to SPIN_MAX_SEARCHERS of them poll their result stamp,
    // more than that sleep in hipStreamSynchronize (wait_result)
    static constexpr int SPIN_MAX_SEARCHERS = 2;
    static constexpr int SPIN_MAX_MS = 200;
    mutable std::atomic<int> active_searches_{0};
    mutable std::atomic<int> last_scan_variant_{0}, last_scan_grid_{0}, last_scan_qarg_{0};
    mutable std::atomic<int> last_filter_[6] = {};
    mutable std::atomic<uint64_t> last_rbatch_[4] = {};
    mutable std::atomic<uint64_t> last_fbatch_[4] = {};
    mutable std::atomic<uint64_t> last_mbatch_[5] = {};
    std::atomic<int> masked_batch_{2};  // MASKED_BATCH_AUTO
    mutable std::atomic<uint64_t> last_gbatch_[4] = {};
    std::atomic<int> grouped_batch_{2};  // GROUPED_BATCH_AUTO
    mutable std::atomic<uint64_t> last_mmrbatch_[4] = {};
    std::atomic<int> mmr_batch_{2};  // MMR_BATCH_AUTO
    std::atomic<uint64_t> last_delete_[6] = {};
    std::atomic<uint64_t> last_update_[7] = {};
    mutable std::mutex prof_mu_;
    mutable uint64_t prof_n_ = 0;
    mutable double prof_ms_ = 0.0;
    mutable uint64_t prof_bytes_ = 0;
};

// NEW: f32 embeddings [n, dim] (host or device) -> widened, optionally L2-normalised f64 rows on the
// device with the arithmetic of src/embeddings.rs:171-179, appended through `append(ids, device rows, count)`.
int add_embeddings_f32(int device, uint64_t dim, const uint64_t* ids, const float* emb, uint64_t n, bool normalize,
                       bool emb_on_device, const std::function<int(const uint64_t*, const double*, uint64_t)>& append);

// NEW: the query side of the same step (src/client.rs:393-401: embed -> index.search): nq f32 embeddings [nq, dim] (host or
// device) are widened and optionally L2-normalised on the device exactly like add_embeddings_f32 does for rows, then handed
// to `search(device f64 queries, count)` -- for the flat index that is search_batch_device: the batch never visits the host.
int search_embeddings_f32(int device, uint64_t dim, const float* emb, uint64_t nq, bool normalize, bool emb_on_device,
                          const std::function<int(const double*, uint64_t)>& search);

}  // namespace vl
