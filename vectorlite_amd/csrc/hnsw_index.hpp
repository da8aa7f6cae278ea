// hnsw_index.hpp -- host side of the GPU HNSW index: mirror of the reference's
// `impl VectorIndex for HNSWIndex` (src/index/hnsw.rs:363-496) above the device graph walk
// (hnsw.hip).  Rows live in a GpuFlatIndex row store (node index = storage position; deletes are
// tombstones exactly like the reference, src/index/hnsw.rs:400-414).
#pragma once

#include <atomic>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "rwlock.hpp"
#include "flat_index.hpp"
#include "hnsw.hpp"

namespace vl {

// convert_distance_to_similarity(d as f64 / 1000.0, metric) (src/index/hnsw.rs:51-75, :478-479)
double hnsw_score(uint64_t d_u64, int metric);
// the level law: the level of node `node` (insertion position) in an index created with `seed` and `m`, 0 .. HNSW_MAX_LEVEL
int hnsw_level(uint64_t seed, uint64_t node, uint32_t m);

struct HnswParams {
    uint32_t m = 16;                // MAXIMUM_NUMBER_CONNECTIONS   (src/index/hnsw.rs:95-101, default profile)
    uint32_t m0 = 32;               // MAXIMUM_NUMBER_CONNECTIONS_0 (src/index/hnsw.rs:103-109)
    uint32_t ef_construction = 400; // HNSWIndex::new calls Hnsw::new(metric) = the crate's Params::default() (src/index/hnsw.rs:226-244);
                                    // SURVEY 9.5 recalls that default as 400 (crate hnsw 0.11.0 is not in the tree: unverified).
                                    // Rounds 1-3 built with 128 because the beam stopped there; measured at N = 1 M x 384
                                    // (profiles/r04_hnsw_efc_sweep_1m_d384.jsonl): 128 -> 400 lifts the strict-beam recall@10 on
                                    // clustered rows 0.48 -> 0.57 (0.66 -> 0.76 at ef 128), nothing on latent-16 rows, build 3.6 -> 9.1 s
    uint64_t seed = 0;
};

// What ONE walk launch needs besides the graph: a stream, the visited sets of its walks (per walk slot a bitmap over the
// nodes + a log of the nodes it set, hnsw.hip: Visited) and the query / result staging buffers.  Launches borrow one from
// a pool inside the index, so searches from different threads run their walk kernels at the same time (the reference
// searches under RwLock::read, src/client.rs:398) -- nothing is shared between two launches but the read-only graph.
struct WalkScratch {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t* d_bits = nullptr;   // [n_slots, words], all zero between walks
    uint32_t* d_log = nullptr;    // [n_slots, log_cap]
    uint32_t n_slots = 0, words = 0, log_cap = 0;
    double* d_q = nullptr;
    unsigned long long* d_out = nullptr;  // [nq*k ids][nq*k score bits][nq counts], one D2H copy per batch
    unsigned long long* h_out = nullptr;  // pinned mirror
    uint64_t q_cap = 0, out_cap = 0;
    ~WalkScratch();
};

// A walk filter of one HNSW handle (vl_index_hnsw_filter_create): an id filter of the row store (its ascending position
// list; node index = storage position) and the pass bitmap built from it -- bit v set iff node v is in the list AND live.
// The bitmap belongs to the handle's mutation count `built_at`; a call that finds the count moved on builds it again.
struct WalkFilter {
    std::mutex mu;                        // guards everything below (taken after the index lock)
    int device = 0;
    uint64_t store_token = 0;             // the row store's IdFilter; also this filter's token
    uint32_t* d_bits = nullptr;           // [words]
    uint64_t words = 0;
    unsigned long long* d_count = nullptr;
    uint64_t n_pass = 0;                  // bits set
    uint64_t subset_rows = 0;             // rows of the store's list, tombstoned ones included
    uint64_t built_at = ~0ull;
    ~WalkFilter();
};

struct HnswGraphProbe;  // tests/native/hnsw_graph_audit.hip: reads the graph arrays and the scratch pool

class HnswIndex {
public:
    struct CoalesceReq {  // one caller waiting in search() while coalescing is on
        const double* query;
        uint64_t k;
        uint32_t ef;
        uint64_t* out_ids;
        double* out_scores;
        uint64_t* out_n;
        uint64_t out_limit;  // entries the caller's buffers hold
        int rc = 6;  // ERR_DEVICE until the walk answers it
        std::string err = "coalesced walk ended without answering this request";
        bool done = false;
    };
    // concurrent single-query search() calls share walk launches (coalescer.hpp); 0 / 1 = off; on by default (create())
    void set_coalescing(int max_batch, int window_us) { co_.configure(max_batch, window_us, 4096); }
    void coalesce_stats(uint64_t* batches, uint64_t* queries) const { co_.stats(batches, queries); }
    void coalesce_gather(int adaptive, uint64_t* waits, uint64_t* waited_us) const
    {
        if (adaptive >= 0) co_.set_adaptive(adaptive != 0);
        co_.gather_stats(waits, waited_us);
    }

    static int create(uint64_t dim, int metric, const HnswParams& p, int device, HnswIndex** out);
    ~HnswIndex();

    int add(uint64_t id, const double* values, uint64_t len);
    int add_bulk(const uint64_t* ids, const double* values, uint64_t n, bool values_on_device);
    int remove(uint64_t id);
    // n remove() calls under one lock: stops at the first id that does not exist (ERR_NOT_FOUND, the reference's message),
    // the ids before it stay tombstoned -- add_bulk's prefix rule.  *out_nodes = nodes tombstoned.
    int remove_bulk(const uint64_t* ids, uint64_t n, uint64_t* out_nodes);
    // ef == 0: the reference's rule ef = min(k, len) (src/index/hnsw.rs:437,454); ef > 0: own extension
    // out_stride (0 = k): the caller's buffers hold out_stride entries per query -- rows are out_stride apart and at most
    // out_stride results are written per row, while the WALK still runs with the caller's k (ef = min(k, len)): the
    // first out_stride entries of what the uncapped call would return (vl_index_search_cap / _batch_cap)
    int search(const double* query, uint64_t q_len, uint64_t k, int metric, uint32_t ef, uint64_t* out_ids,
               double* out_scores, uint64_t* out_n, uint64_t out_stride = 0) const;
    int search_batch(const double* queries, uint64_t nq, uint64_t q_len, uint64_t k, int metric, uint32_t ef,
                     uint64_t* out_ids, double* out_scores, uint64_t* out_n, uint64_t out_stride = 0) const;
    // NEW (no reference counterpart): walks restricted to the nodes whose id is in a set.  A filter
    // is a token of this handle (never 0, never reused, not cloned, freed with the handle); ids may be unsorted and repeat,
    // ids the index does not hold are ignored.  *out_nodes / filter_nodes: the nodes that pass now (in the set and live).
    int filter_create(const uint64_t* ids, uint64_t n_ids, uint64_t* out_token, uint64_t* out_nodes);
    int filter_nodes(uint64_t token, uint64_t* out_nodes) const;
    int filter_destroy(uint64_t token);
    // search_batch's arguments, errors and outputs; one filter serves every query of the batch.  Returns per query the
    // passing nodes a walk of width ef_walk finds (hnsw_filter_plan.hpp: walk route), or the exact nearest passing rows
    // (exact route).  Never joins a coalesced pass.
    int search_filtered(uint64_t token, const double* queries, uint64_t nq, uint64_t q_len, uint64_t k, int metric, uint32_t ef,
                        uint64_t* out_ids, double* out_scores, uint64_t* out_n, uint64_t out_stride = 0) const;
    // the last search_filtered on this handle that reached the plan: route (0 walk, 1 exact), the walk's list capacity
    // (0 on the exact route), the passing nodes, and the walks whose list was cut at that capacity
    void last_filtered(int* route, uint32_t* cap, uint64_t* pass_nodes, uint64_t* cap_cut_walks) const
    {
        if (route) *route = last_filt_route_.load(std::memory_order_relaxed);
        if (cap) *cap = last_filt_cap_.load(std::memory_order_relaxed);
        if (pass_nodes) *pass_nodes = last_filt_pass_.load(std::memory_order_relaxed);
        if (cap_cut_walks) *cap_cut_walks = last_filt_cut_.load(std::memory_order_relaxed);
    }
    uint64_t len() const;
    uint64_t dimension() const { return dim_; }
    int device() const { return device_; }
    int metric() const { return metric_; }
    int get_vector(uint64_t id, double* out) const;
    int max_id(uint64_t* out) const;
    uint64_t graph_nodes() const { return n_nodes_; }
    // #[derive(Clone)] on HNSWIndex (persistence clones the wrapper, src/persistence.rs:118): a deep copy of
    // the rows and of the device graph, tombstones included.
    // queries walked and Metric::distance evaluations made by them since creation (SURVEY 8(d) C4:
    // navigation evaluations read f32 rows, the final beam's exact evaluations f64 rows)
    void walk_stats(uint64_t* queries, uint64_t* distance_evals) const;
    // beam floor of searches that name no ef (0 = the reference's strict ef = min(k, len)); at most HNSW_MAX_EF
    void set_min_beam(uint32_t b) { min_beam_.store(b > (uint32_t)HNSW_MAX_EF ? (uint32_t)HNSW_MAX_EF : b); }
    uint32_t min_beam() const { return min_beam_.load(); }
    // how walks navigate (opt-in): NAV_F32 (default) = f32 navigation, the final beam re-scored with the exact u64;
    // NAV_REFERENCE = every evaluation the exact u64, ties in first-seen order (launch_hnsw_search_ref).  Read once
    // per launch.  Pinned for walks only: a beam past HNSW_MAX_EF is answered by the exact scan in either mode.
    // Like min_beam, a clone or a reloaded index starts in NAV_F32.
    static constexpr int NAV_F32 = 0, NAV_REFERENCE = 1;
    void set_navigation(int mode) { nav_.store(mode == NAV_REFERENCE ? NAV_REFERENCE : NAV_F32); }
    int navigation() const { return nav_.load(); }
    int clone(HnswIndex** out) const;
    // live rows in node (insertion) order: the `vector_values` member of the serialised form
    int export_rows(uint64_t* out_ids, double* out_values) const;
    // the graph as it stands (every node, tombstoned ones included): for inspection and CPU-side walks
    void graph_info(uint64_t* n_nodes, uint32_t* entry, int* max_level, uint32_t* m, uint32_t* m0, uint64_t* upper_slots) const;
    int graph_export(uint8_t* level, uint32_t* upper_off, uint32_t* cnt0, uint32_t* nbr0, uint32_t* cntU, uint32_t* nbrU,
                     uint64_t* node_ids, uint8_t* live, double* rows) const;
    const HnswParams& params() const { return params_; }
    // The inverse of graph_export on an EMPTY index (no node yet, created with the graph's dim, metric, m, m0 and seed):
    // node i is storage position i, its lists are taken as given (entry order included), levels and upper offsets are
    // derived from the level law (n_upper must be their total), entry / max_level follow.  The lists are validated on
    // the host first (hnsw_import_plan.hpp: G3, G4); the edge distances and the in-degree counter are recomputed on the
    // device.  Among LIVE nodes an id may appear once (ERR_DUP_ID).  *out_orphans (optional): nodes without an incoming
    // layer-0 edge, counted as the audit counts them (none when n < 2).  Every refusal and every failure leaves the
    // index as empty as it was and still accepting adds.
    int graph_import(uint64_t n, const uint64_t* node_ids, const uint8_t* live, const double* rows, bool rows_on_device,
                     const uint32_t* cnt0, const uint32_t* nbr0, uint64_t n_upper, const uint32_t* cntU, const uint32_t* nbrU,
                     uint64_t* out_orphans);
    // milliseconds of the last graph_import: host validation, row ingest, uploads, edge-key kernel, in-degree kernel
    // (HIP events around the kernels, the host clock around the rest); zeros before the first import
    void last_import_ms(double out[5]) const;

private:
    friend struct HnswGraphProbe;
    HnswIndex(uint64_t dim, int metric, const HnswParams& p, int device);
    int ensure_graph(uint64_t nodes, uint64_t upper_slots);
    int zero_graph_counters();  // graph_import, on an index without nodes
    HnswGraphView view() const;
    HnswGraphView view(const WalkScratch* ws) const;
    WalkScratch* acquire_scratch(uint64_t walks) const;  // nullptr + last_error on failure
    void release_scratch(WalkScratch* ws) const;
    void drop_scratch_pool();                             // the graph's capacity changed (caller holds the unique lock)
    int ensure_io(WalkScratch* ws, uint64_t nq, uint64_t k) const;
    int search_exact_fallback(const double* query, uint64_t k, uint64_t* out_ids, double* out_scores, uint64_t* out_n,
                              uint64_t out_limit) const;
    int find_walk_filter(uint64_t token, std::shared_ptr<WalkFilter>* out) const;
    int refresh_walk_filter(WalkFilter* f) const;  // mu_ held (shared or unique), f->mu held: builds the bitmap if stale
    // the exact route of one query; mu_ held (shared), n_pass > 0, tombs = tombstoned rows of the filter's subset
    int search_filtered_exact(const WalkFilter* f, uint64_t tombs, const double* query, uint64_t k, uint64_t* out_ids,
                              double* out_scores, uint64_t* out_n, uint64_t out_limit) const;

    const uint64_t dim_;
    const int metric_;
    const HnswParams params_;
    const int device_;
    std::unique_ptr<GpuFlatIndex> store_;
    mutable RwLock mu_;
    hipStream_t stream_ = nullptr;  // mutators (graph growth, level upload, tombstones)
    mutable std::mutex pool_mu_;
    mutable std::condition_variable pool_cv_;
    mutable std::vector<std::unique_ptr<WalkScratch>> pool_all_;
    mutable std::vector<WalkScratch*> pool_free_;
    mutable size_t pool_pending_ = 0;    // scratches being allocated (slot and bytes already counted)
    mutable uint64_t pool_bytes_ = 0;    // visited-set bytes of pool_all_ + pending

    // device graph
    uint32_t* d_nbr0_ = nullptr;
    unsigned long long* d_dist0_ = nullptr;
    uint32_t* d_cnt0_ = nullptr;
    uint8_t* d_level_ = nullptr;
    uint32_t* d_upper_off_ = nullptr;
    uint32_t* d_nbrU_ = nullptr;
    unsigned long long* d_distU_ = nullptr;
    uint32_t* d_cntU_ = nullptr;
    uint32_t* d_lock_ = nullptr;
    uint32_t* d_indeg0_ = nullptr;
    uint64_t g_cap_ = 0, u_cap_ = 0;

    // host bookkeeping
    std::vector<uint8_t> level_;
    std::vector<uint32_t> upper_off_;
    uint64_t n_upper_ = 0;
    uint32_t entry_ = HNSW_NONE;
    int max_level_ = -1;
    uint64_t n_nodes_ = 0;
    std::unordered_map<uint64_t, uint32_t> id_to_node_;  // live ids only (id_to_index, src/index/hnsw.rs:205)
    std::vector<uint64_t> node_id_;
    std::vector<uint8_t> live_;
    uint64_t live_count_ = 0;
    double import_ms_[5] = {0, 0, 0, 0, 0};  // last graph_import, see last_import_ms()
    uint64_t mutations_ = 0;  // add / delete / import calls so far (a walk filter's staleness test: tombstoning counts)
    mutable std::mutex wfilters_mu_;  // the filter table; never held while mu_ or a filter's mutex is taken
    std::unordered_map<uint64_t, std::shared_ptr<WalkFilter>> wfilters_;
    mutable std::atomic<int> last_filt_route_{0};
    mutable std::atomic<uint32_t> last_filt_cap_{0};
    mutable std::atomic<uint64_t> last_filt_pass_{0}, last_filt_cut_{0};

    std::atomic<uint32_t> min_beam_{0};  // 0 = the reference's strict ef = min(k, len); a wider floor is opt-in
    std::atomic<int> nav_{NAV_F32};      // walk navigation; the reference's u64 order is opt-in
    mutable std::atomic<uint64_t> stat_queries_{0}, stat_evals_{0};  // stat_evals_: the exact-fallback's share only
    mutable Coalescer<CoalesceReq> co_;

    unsigned long long* d_node_id_ = nullptr;      // [g_cap_] node -> caller's id (device copy of node_id_)
    uint8_t* d_live_ = nullptr;                    // [g_cap_] 0 = tombstoned
    unsigned long long* d_stat_evals_ = nullptr;   // distance evaluations of all query walks
};

}  // namespace vl
